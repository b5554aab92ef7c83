"""Per-clip frame lengths of the Keras hybrid family on the MI355X (DESIGN.md §2 "Frame lengths").

Module parity: every module with a masked operation (the three Conv1DBlocks of a stage, both attentions, the Squeezeformer ConvModule) alone
through the ishara_debug_module_*_ex probes against the fp64 restatement of tests/frame_mask_parity.py — y, dx, every parameter gradient,
the implied batch statistics — at module_parity's bounds.  Shapes: cfg2 (d256, H8, dh32) at T = 72, B = 3 with lengths (72, 37, 9) and
(72, 0, 1), f32 (the masked lane-split attention) and bf16 (the masked MFMA attention), dropout 0 and 0.2; the d512 / dh64 model at T = 136,
lengths (129, 64), bf16: both MFMA head dims, a partial last key chunk, a length below one chunk, an empty clip.

Exactness: rows t >= n_b of a module's input redrawn from N(0, 100^2) leave its output rows t < n_b bit-equal.  NULL lengths are the plain
entry points bit for bit; lengths all T agree with the unmasked call inside the module bounds (other kernels run).  The whole model in f32
against the restatement chained through the oracle's forward, at test_model_gpu.py's bounds.  ishara_frame_lengths against numpy, exactly."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import frame_mask_parity as FM
import module_parity as MP
from ishara_amd import _lib, frame_lengths, get_model
from oracle import ishara_oracle as O
from test_model_gpu import _log_observed

pytestmark = pytest.mark.gpu
_cache = {}


def _model(shape, dtype, dropout, B):
    key = (shape, dtype, dropout, B)
    if _cache.get("key") != key:
        _cache.clear()
        torch.cuda.empty_cache()
        os.environ["ISHARA_WS_GUARD"] = "1"
        try:
            model = get_model(**FM.SHAPES[shape], dropout_rate=dropout, head_dropout=0.4 if dropout > 0 else 0.0,
                              conformer_attn_dropout=0.1 if dropout > 0 else 0.0, dtype=dtype, max_batch=B, seed=3)
        finally:
            os.environ.pop("ISHARA_WS_GUARD", None)
        W = MP.perturbed(model.get_weights(), dtype)
        model.set_weights(W)
        _cache.update(key=key, model=model, W=W, flat=model.params.clone())
    return _cache["model"], _cache["W"], _cache["flat"]


def _run(model, flat, name, i, x, dy, seed, lens):
    """one training forward + backward of module i through the probe (lens None: the plain probe) -> module_parity's `got`"""
    model.params.copy_(flat)
    y = model.module_forward(i, x, training=True, seed=seed, frame_lengths=lens)
    dx = model.module_backward(i, dy, frame_lengths=lens)
    torch.cuda.synchronize()
    _lib.check(model._lib.ishara_workspace_guard_check(model._h), "workspace guard (a kernel wrote outside its buffer)")
    gflat = model.grads[:model.n_train].cpu().numpy()
    pflat = model.params.cpu().numpy()
    mine = np.zeros(model.n_train, bool)
    for n, s, o, t in model.entries:
        if t and MP.owns(name, n):
            mine[o:o + int(np.prod(s))] = True
    assert int(np.count_nonzero(gflat[~mine])) == 0, f"gradient elements outside {name}'s entries are not zero"
    got = dict(y=y.cpu().numpy(), dx=dx.cpu().numpy(),
               grads={n: gflat[o:o + int(np.prod(s))].reshape(s) for n, s, o, t in model.entries if t and MP.owns(name, n)},
               stats={n: pflat[o:o + int(np.prod(s))].reshape(s) for n, s, o, t in model.entries if not t and MP.owns(name, n)}, loss=None)
    assert np.isfinite(got["y"]).all() and np.isfinite(got["dx"]).all() and np.isfinite(gflat).all()
    model.params.copy_(flat)
    return got


def _module_cases():
    out = []
    for dtype in ("f32", "bf16"):
        for dropout in (0.0, 0.2):
            for lens_id in ("ragged", "edge"):
                out.extend(("cfg2", dtype, dropout, lens_id, n) for n in FM.MODULES)
    out.extend(("d512", "bf16", 0.2, "d512", n) for n in FM.MODULES)
    return out


def _lens_of(lens_id):
    return FM.LENS_D512 if lens_id == "d512" else FM.LENS[lens_id]


@pytest.mark.parametrize("shape,dtype,dropout,lens_id,name", _module_cases(), ids=lambda v: str(v).replace("/", ".") if not isinstance(v, float) else f"drop{v}")
def test_module_with_lengths_matches_fp64(shape, dtype, dropout, lens_id, name):
    lens = _lens_of(lens_id)
    B = len(lens)
    model, W, flat = _model(shape, dtype, dropout, B)
    cfg = FM.ocfg(shape, dropout)
    assert model.module_names() == MP.expected_modules(cfg)
    i, first, x, dy, seed = FM.case_inputs(cfg, name, B, dtype, dropout)
    assert (i, first) == (model.module_names().index(name), model._module_info(i)[3])
    ref = FM.reference(name, cfg, W, x, dy, seed, first, lens)
    assert ref["sites_used"] == model._module_info(i)[4]
    kind = MP.module_kind(name)
    bound = FM.bounds(kind, dtype, shape, lens_id)
    got = _run(model, flat, name, i, x, dy, seed, lens)
    obs, bad = MP.compare(name, dtype, B, cfg.T, got, ref, W, bound)
    _log_observed(dict(test="frame_mask_module", module=name, kind=kind, shape=shape, dtype=dtype, dropout=dropout, lens=list(lens), **obs))
    print(f"observed {obs}")
    if kind == "mha":          # a clip without frames: its attention adds nothing, the output rows are the residual input
        for b, n in enumerate(lens):
            if n == 0 and dropout == 0.0:
                assert np.abs(got["y"][b] - x[b]).max() <= 1e-6 * np.abs(x[b]).max()
    assert not bad, "\n".join(bad)


EXACT = [("squeezeformer_0/mha", True, 0.2), ("squeezeformer_0/mha", False, 0.0), ("conformer_0/mha", True, 0.2), ("squeezeformer_0/conv", True, 0.0),
         ("squeezeformer_0/conv", False, 0.0), ("convsqueeze_0_1", False, 0.0), ("convsqueeze_0_3", False, 0.0)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,training,dropout", EXACT, ids=lambda v: str(v).replace("/", "."))
def test_padding_rows_do_not_reach_the_valid_rows(dtype, name, training, dropout):
    """the module's input rows t >= n_b redrawn from N(0, 100^2): the output rows t < n_b are bit-equal (a Conv1DBlock: eval mode, where the
    BatchNorm uses its moving statistics; in training its batch statistics see the padding by design)"""
    lens = FM.LENS["ragged"]
    model, W, flat = _model("cfg2", dtype, dropout, len(lens))
    cfg = FM.ocfg("cfg2", dropout)
    i, first, x, dy, seed = FM.case_inputs(cfg, name, len(lens), dtype, dropout)
    g = np.random.default_rng(77)
    x2 = x.copy()
    for b, n in enumerate(lens):
        x2[b, n:] = MP.round_to(100.0 * g.standard_normal(x2[b, n:].shape), dtype)
    assert np.abs(x2 - x).max() > 50
    ys = []
    for xin in (x, x2):
        model.params.copy_(flat)
        ys.append(model.module_forward(i, xin, training=training, seed=seed, frame_lengths=lens).cpu().numpy())
    model.params.copy_(flat)
    for b, n in enumerate(lens):
        assert np.array_equal(ys[0][b, :n], ys[1][b, :n]), f"clip {b}: rows below {n} moved with the padding"
    assert not np.array_equal(ys[0][1, lens[1]:], ys[1][1, lens[1]:])      # (the padding rows themselves do change)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", FM.MODULES, ids=lambda v: v.replace("/", "."))
def test_lengths_all_T_agree_with_the_unmasked_call(dtype, name):
    B, T = FM.B_SMALL, FM.T_SMALL
    model, W, flat = _model("cfg2", dtype, 0.2, B)
    cfg = FM.ocfg("cfg2", 0.2)
    i, first, x, dy, seed = FM.case_inputs(cfg, name, B, dtype, 0.2)
    plain = _run(model, flat, name, i, x, dy, seed, None)
    full = _run(model, flat, name, i, x, dy, seed, [T] * B)
    obs, bad = MP.compare(name, dtype, B, T, full, plain, W, FM.bounds(MP.module_kind(name), dtype, "cfg2"))
    print(f"observed {obs}")
    assert not bad, "\n".join(bad)
    over = _run(model, flat, name, i, x, dy, seed, [T + 1000] * B)          # clamped to T on the device
    assert np.array_equal(over["y"], full["y"]) and np.array_equal(over["dx"], full["dx"])


SMALL = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(48, 36))


def _small(dtype="f32", dropout=0.2, B=4):
    model = get_model(**SMALL, dropout_rate=dropout, head_dropout=0.4 if dropout else 0.0, conformer_attn_dropout=0.1 if dropout else 0.0,
                      dtype=dtype, max_batch=B, seed=3)
    W = MP.perturbed(model.get_weights(), "f32")
    model.set_weights(W)
    cfg = O.Config(dropout_rate=dropout, head_dropout=0.4 if dropout else 0.0, conformer_attn_dropout=0.1 if dropout else 0.0, **SMALL)
    return model, W, cfg


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_null_lengths_are_the_plain_entry_points_bit_for_bit(dtype):
    model, W, cfg = _small(dtype)
    flat = model.params.clone()
    x, y = O.synthetic_batch(cfg, 4, seed=1)
    a = model(x).cpu().numpy()
    b = model(x, frame_lengths=None).cpu().numpy()
    assert np.array_equal(a, b)
    loss, logits = model.loss_and_gradients(x, y, seed=11)
    g0, l0, s0 = model.grads.clone(), logits.clone(), model.params.clone()
    model.params.copy_(flat)
    xd = torch.from_numpy(x).to(model.device)
    yd = torch.from_numpy(y).to(model.device)
    lg = torch.empty_like(l0)
    lib = model._lib
    _lib.check(lib.ishara_forward_ex(model._h, _lib.ptr(xd), 4, _lib.ptr(lg), 1, C.c_uint32(11), None, _lib.stream()), "ishara_forward_ex")
    _lib.check(lib.ishara_loss_backward_ex(model._h, _lib.ptr(lg), _lib.ptr(yd), 4, _lib.ptr(model._loss_buf), _lib.ptr(model._nll_buf), C.c_float(1.0), None,
                                           _lib.stream()), "ishara_loss_backward_ex")
    torch.cuda.synchronize()
    assert torch.equal(lg, l0) and torch.equal(model.grads, g0) and torch.equal(model.params, s0)


def test_whole_model_with_lengths_matches_fp64():
    """loss_and_gradients(x, y, frame_lengths=) in f32 against the restatement chained through oracle.forward's structure, at test_model_gpu.py's bounds"""
    model, W, cfg = _small("f32")
    x, y = O.synthetic_batch(cfg, 4, seed=1)
    lens = (48, 23, 0, 7)
    loss_t, logits_t = model.loss_and_gradients(x, y, seed=4242, frame_lengths=torch.tensor(lens, device=model.device))
    torch.cuda.synchronize()
    loss, logits, grads, W_after = float(loss_t.item()), logits_t.cpu().numpy(), model.get_gradients(), model.get_weights()
    ref_loss, ref_logits, ref_grads, ref_stats = FM.loss_and_grads(W, x, y, cfg, lens, training=True, seed=4242)
    plain = O.loss_and_grads(W, x, y, cfg, training=True, seed=4242, dtype=torch.float64)
    assert np.abs(ref_logits - plain[1]).max() > 1e-2          # the lengths matter on this batch
    lerr = float(np.abs(logits - ref_logits).max())
    gscale = max(float(np.abs(v).max()) for v in ref_grads.values())
    bad, worst = [], 0.0
    for n, rg in ref_grads.items():
        if np.abs(rg).max() < 1e-6 * gscale:
            if np.abs(grads[n]).max() > 1e-3 * gscale: bad.append((n, float(np.abs(grads[n]).max() / gscale)))
            continue
        e = float(np.abs(grads[n] - rg).max() / np.abs(rg).max())
        worst = max(worst, e)
        if e > 1e-3: bad.append((n, e))
    _log_observed(dict(test="frame_mask_model", dtype="f32", logits_max_abs_err=lerr, loss_rel_err=abs(loss - ref_loss) / abs(ref_loss), worst_grad_err=worst))
    print(f"logits {lerr:.3e} loss {abs(loss - ref_loss) / abs(ref_loss):.3e} worst grad {worst:.3e}")
    assert lerr <= 1e-4, f"logits max-abs-err {lerr:.3e}"
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss) + 1e-4, (loss, ref_loss)
    assert not bad, f"gradient mismatch: {sorted(bad, key=lambda t: -t[1])[:8]}"
    for n, rs in ref_stats.items():
        assert np.abs(W_after[n] - rs).max() <= 1e-4 * (1 + np.abs(rs).max()), n


def test_training_surface_takes_lengths_and_a_disagreeing_backward_is_refused():
    """train_on_batch (plain and the accumulating / clipping path), fit and evaluate over (x, y, frame_lengths) batches; a backward call must be
    given lengths exactly when its training forward was"""
    model, W, cfg = _small("bf16")
    x, y = O.synthetic_batch(cfg, 4, seed=1)
    fl = np.array([48, 30, 12, 5])
    l1 = float(model.train_on_batch(x, y, seed=5, frame_lengths=fl).item())
    model.optimizer.accumulate_steps, model.optimizer.global_clipnorm = 2, 1.0
    for _ in range(2):
        l2 = float(model.train_on_batch(x, y, frame_lengths=list(fl)).item())
    assert np.isfinite([l1, l2]).all() and model.grad_stats()["nonfinite"] == 0
    model.optimizer.accumulate_steps, model.optimizer.global_clipnorm = 1, None
    hist = model.fit([(x, y, fl), (x, y)], validation_data=[(x, y, fl)], epochs=1, verbose=0)
    assert np.isfinite(hist.history["loss"][0]) and np.isfinite(hist.history["val_loss"][0])
    a, b = model.evaluate([(x, y, fl)]), model.evaluate([(x, y)])
    assert np.isfinite([a, b]).all() and a != b
    # disagreement, both ways
    lib, fld = model._lib, torch.from_numpy(fl).to(model.device, torch.int32)
    logits = model(x, training=True, seed=1, frame_lengths=fld)
    yd = torch.from_numpy(y).to(model.device)
    before = model.grads.clone()
    rc = lib.ishara_loss_backward(model._h, _lib.ptr(logits), _lib.ptr(yd), 4, None, None, C.c_float(1.0), _lib.stream())
    assert rc != 0 and "frame lengths" in lib.ishara_last_error().decode()
    logits = model(x, training=True, seed=1)
    rc = lib.ishara_loss_backward_ex(model._h, _lib.ptr(logits), _lib.ptr(yd), 4, None, None, C.c_float(1.0), _lib.ptr(fld), _lib.stream())
    assert rc != 0 and "frame lengths" in lib.ishara_last_error().decode()
    i = model.module_names().index("squeezeformer_0/conv")
    xm = torch.zeros(4, 48, 64, device=model.device)
    model.module_forward(i, xm, training=True, seed=1, frame_lengths=fld)
    with pytest.raises(_lib.IsharaError, match="frame lengths"):
        model.module_backward(i, xm)
    torch.cuda.synchronize()
    assert torch.equal(model.grads, before)          # a refused call launches nothing


@pytest.mark.parametrize("T", [8, 512])
def test_frame_lengths_kernel_equals_numpy(T):
    g = np.random.default_rng(T)
    B, F = 9, 36
    x = np.zeros((B, T, F), np.float32)
    x[1, T - 1, F - 1] = 1e-30                       # one non-zero feature in the last frame
    x[2, : T // 2] = g.standard_normal((T // 2, F)); x[2, 1] = 0.0      # an interior zero frame stays valid
    x[3, 0, 0] = -0.0                                # a negative zero is a zero: the clip is empty
    x[4, 0, 5] = 3.0                                 # only the first frame
    x[5] = g.standard_normal((T, F))
    x[6, : T - 3] = g.standard_normal((T - 3, F))
    x[7, T // 3, 2] = np.nan                         # a NaN is not zero
    x[8, :5] = g.standard_normal((5, F)); x[8, 4, :] = 0.0; x[8, 4, F - 1] = 2.0
    want = FM.frame_lengths_np(x)
    assert want.tolist()[:5] == [0, T, T // 2, 0, 1]
    got = frame_lengths(torch.from_numpy(x).cuda())
    assert got.dtype == torch.int32 and got.cpu().numpy().tolist() == want.tolist()
