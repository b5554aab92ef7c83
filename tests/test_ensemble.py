"""CPU: model ensembling (ishara_amd/ensemble.py, csrc/logits_combine.hip) as far as it goes without a device: the properties of the fp64
reference every other ensemble test measures against, the refusals of normalise_weights, every refusal of ishara_logits_combine (before any
HIP call: all device pointers are NULL or made up, and the stream is NULL) and EnsembleTFLiteModel's constructor refusals."""
import ctypes as C

import numpy as np
import pytest

from ishara_amd import make_config
from ishara_amd.ensemble import EnsembleTFLiteModel, combine_reference, normalise_weights
from ishara_amd.model import Model

N = None
NAME = "ishara_logits_combine"


def _lsm(x):
    x = np.asarray(x, np.float64)
    d = x - x.max(-1, keepdims=True)
    return d - np.log(np.exp(d).sum(-1, keepdims=True))


def _logits(M, B=3, T=7, Cn=60, seed=0):
    g = np.random.default_rng(seed)
    return [(2.0 * g.standard_normal((B, T, Cn))).astype(np.float32) for _ in range(M)]


# ---------------------------------------------------------------------------------------------------- the reference's properties
@pytest.mark.parametrize("mode", ["log_linear", "linear"])
def test_one_model_is_its_log_softmax(mode):
    (x,) = _logits(1)
    assert np.abs(combine_reference([x], mode=mode) - _lsm(x)).max() < 1e-12
    # one weight that is not 1: a sharpening exponent of the product of experts, nothing to the mixture
    assert np.abs(combine_reference([x], [0.3], mode) - (_lsm(x) if mode == "linear" else _lsm(_lsm(x) * 0.3))).max() < 1e-12
    assert np.abs(combine_reference([x], mode=mode, temperatures=[2.0]) - _lsm(x.astype(np.float64) / 2.0)).max() < 1e-12


@pytest.mark.parametrize("mode", ["log_linear", "linear"])
def test_one_hot_weight_returns_that_model(mode):
    xs = _logits(4, seed=1)
    xs[0] = np.full_like(xs[0], np.nan)                       # a model whose weight is not > 0 is not read
    got = combine_reference(xs, [0, 0, 1, 0], mode)
    assert np.abs(got - _lsm(xs[2])).max() < 1e-12


@pytest.mark.parametrize("mode", ["log_linear", "linear"])
def test_permuting_models_with_their_weights_changes_nothing(mode):
    xs, w, t = _logits(5, seed=2), np.array([0.1, 0.3, 0.0, 0.4, 0.2]), np.array([1.0, 0.5, 2.0, 1.5, 0.8])
    base = combine_reference(xs, w, mode, t)
    p = np.random.default_rng(3).permutation(5)
    assert np.abs(combine_reference([xs[i] for i in p], w[p], mode, t[p]) - base).max() < 1e-12


@pytest.mark.parametrize("mode", ["log_linear", "linear"])
@pytest.mark.parametrize("w", [None, [0.5, 0.25, 0.25], [3.0, 1.0, 0.5], [0.0, 0.0, 0.0]])
def test_every_row_is_normalised_whatever_the_weights_sum_to(mode, w):
    out = combine_reference(_logits(3, seed=4), w, mode)
    assert np.abs(np.log(np.exp(out).sum(-1))).max() < 1e-12
    if w is not None and not any(w):
        assert np.abs(out + np.log(60.0)).max() < 1e-12       # no weight > 0: the uniform row


def test_the_two_modes_differ_where_they_must():
    """two confident models that disagree: the product of experts keeps what both allow, the mixture keeps both peaks"""
    a, b = np.zeros((1, 1, 4), np.float32), np.zeros((1, 1, 4), np.float32)
    a[..., 0], a[..., 2], b[..., 1], b[..., 2] = 6.0, 4.0, 6.0, 4.0
    pe, mix = combine_reference([a, b], mode="log_linear")[0, 0], combine_reference([a, b], mode="linear")[0, 0]
    assert np.argmax(pe) == 2 and np.argmax(mix) in (0, 1) and abs(mix[0] - mix[1]) < 1e-12
    assert np.abs(pe - mix).max() > 1.0
    p = 0.5 * np.exp(_lsm(a)) + 0.5 * np.exp(_lsm(b))
    assert np.abs(mix - np.log(p[0, 0])).max() < 1e-12        # the mixture, computed directly
    assert np.abs(pe - _lsm(0.5 * _lsm(a) + 0.5 * _lsm(b))[0, 0]).max() < 1e-12


@pytest.mark.parametrize("mode", ["log_linear", "linear"])
def test_rows_past_a_clips_end_are_plus_zero(mode):
    xs = _logits(2, B=6, T=5, seed=5)
    fl = [0, 1, 4, 5, 10, -3]
    out = combine_reference(xs, None, mode, None, fl)
    full = combine_reference(xs, None, mode)
    for b, tb in enumerate([0, 1, 4, 5, 0, 0]):
        assert np.array_equal(out[b, :tb], full[b, :tb])
        assert (out[b, tb:] == 0).all() and not np.signbit(out[b, tb:]).any()
    with pytest.raises(ValueError):
        combine_reference(xs, None, mode, None, [1, 2])
    with pytest.raises(ValueError):
        combine_reference(xs, mode="product")


def test_the_linear_mode_does_not_underflow():
    """every model far below the others' support: exp(lp) underflows in fp64 only without the max-subtracted form"""
    a, b = np.zeros((1, 1, 3), np.float32), np.zeros((1, 1, 3), np.float32)
    a[..., 0], b[..., 0] = 2000.0, 1900.0
    out = combine_reference([a, b], [0.5, 0.5], "linear")
    assert np.isfinite(out).all() and out[0, 0, 1] < -1800


# ---------------------------------------------------------------------------------------------------- normalise_weights
def test_normalise_weights():
    assert normalise_weights(None, 4).tolist() == [0.25] * 4 and normalise_weights(None, 4).dtype == np.float32
    w = normalise_weights([1, 2, 5], 3)
    assert w.dtype == np.float32 and np.array_equal(w, (np.array([1, 2, 5]) / 8.0).astype(np.float32))
    assert np.array_equal(normalise_weights([0, 3, 0], 3), np.array([0, 1, 0], np.float32))
    for bad in ([1, 2], [1, 2, 3, 4], [[1, 2, 3]], [1, -1e-9, 1], [1, float("nan"), 1], [1, float("inf"), 1], [0, 0, 0]):
        with pytest.raises(ValueError):
            normalise_weights(bad, 3)
    with pytest.raises(ValueError):
        normalise_weights(None, 0)


# ---------------------------------------------------------------------------------------------------- ishara_logits_combine's refusals
def _refused(lib, rc, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, "the call was accepted"
    assert msg.startswith(NAME + ":"), f"the error is not the entry point's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{msg!r} does not say {w!r}"


def _call(lib, ptrs="good", **kw):
    """one call with made-up 4-byte aligned addresses (a refused call dereferences nothing); `kw` replaces single arguments"""
    v = dict(M=2, B=2, T=16, C=60, mode=0, weights=C.c_void_p(4096), inv_temp=N, frame_len=N, out=C.c_void_p(1 << 24))
    assert set(kw) <= set(v), kw
    v.update(kw)
    if ptrs == "good":
        ptrs = [(1 << 20) + m * (1 << 16) for m in range(max(v["M"], 1))]
    arr = None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)
    return lib.ishara_logits_combine(N, arr, v["M"], v["B"], v["T"], v["C"], v["weights"], v["inv_temp"], v["mode"], v["frame_len"], v["out"], N)


@pytest.mark.parametrize("kw,words", [(dict(M=0), ("M=0", "1..8")), (dict(M=9), ("M=9", "1..8")), (dict(M=-1), ("M=-1",)),
                                      (dict(C=1), ("C=1", "2..64")), (dict(C=65), ("C=65", "2..64")), (dict(T=0), ("T=0", "1..4096")),
                                      (dict(T=4097), ("T=4097", "1..4096")), (dict(B=-1), ("B=-1",)), (dict(mode=2), ("mode 2",)), (dict(mode=-1), ("mode -1",))],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_logits_combine_refuses_shapes_and_modes(lib, kw, words):
    _refused(lib, _call(lib, **kw), *words)


def test_logits_combine_refuses_null_buffers(lib):
    _refused(lib, _call(lib, ptrs=None), "null logits")
    _refused(lib, _call(lib, ptrs=[1 << 20, None]), "null logits[1]")
    _refused(lib, _call(lib, ptrs=[None, 1 << 20]), "null logits[0]")
    _refused(lib, _call(lib, weights=N), "null weights")
    _refused(lib, _call(lib, out=N), "null out")


def test_logits_combine_refuses_misaligned_buffers(lib):
    for off in (1, 2, 3):
        _refused(lib, _call(lib, ptrs=[1 << 20, (1 << 21) + off]), "misaligned", "4-byte")
        _refused(lib, _call(lib, weights=C.c_void_p(4096 + off)), "misaligned", "4-byte")
        _refused(lib, _call(lib, inv_temp=C.c_void_p(8192 + off)), "misaligned", "4-byte")
        _refused(lib, _call(lib, frame_len=C.c_void_p(12288 + off)), "misaligned", "4-byte")
        _refused(lib, _call(lib, out=C.c_void_p((1 << 24) + off)), "misaligned", "4-byte")


def test_logits_combine_refuses_an_output_that_overlaps_an_input(lib):
    nbytes = 2 * 16 * 60 * 4
    a, b = 1 << 20, 1 << 21
    for out, m in ((a, 0), (b, 1), (a + nbytes - 4, 0), (b - nbytes + 4, 1), (b + 4, 1)):
        _refused(lib, _call(lib, ptrs=[a, b], out=C.c_void_p(out)), f"out overlaps logits[{m}]")


def test_logits_combine_of_an_empty_batch_is_a_no_op(lib):
    """B == 0 returns 0 without a launch, whatever the pointers; the shape checks still hold"""
    assert _call(lib, ptrs=None, B=0, weights=N, out=N) == 0
    _refused(lib, _call(lib, B=0, M=9), "M=9")


# ---------------------------------------------------------------------------------------------------- EnsembleTFLiteModel's constructor
def _model(**kw):
    v = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4)
    v.update(kw)
    return Model(make_config(**v), device=None)


def test_ensemble_constructor_refusals_that_need_no_device():
    a = _model()
    for models, kw, word in (([], {}, "0 models"), ([a] * 9, {}, "9 models"),
                             ([a, _model(input_shape=(128, 276))], {}, "share T"), ([a, _model(num_classes=32)], {}, "share C"),
                             ([a, _model(max_label_len=32)], {}, "share max_label_len"), ([a, _model(input_shape=(176, 36))], {}, "F=36"),
                             ([a, _model(max_batch=2)], dict(batch_size=3), "smallest max_batch"), ([a], dict(batch_size=0), "batch_size 0"),
                             ([a, a], dict(weights=[1.0]), "weights"), ([a, a], dict(weights=[0.0, 0.0]), "all zero"), ([a, a], dict(mode="sum"), "mode"),
                             ([a, a], dict(temperatures=[1.0, 0.0]), "temperatures"), ([a, a], dict(temperatures=[1.0]), "temperatures")):
        with pytest.raises(ValueError, match=word):
            EnsembleTFLiteModel(models, batch_size=kw.pop("batch_size", 2), **kw)
    with pytest.raises(ValueError, match="no device"):      # everything else is in order: the base class asks for the device
        EnsembleTFLiteModel([a, _model(num_conv_squeeze_blocks=2, dtype="f32")], batch_size=2)
