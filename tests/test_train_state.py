"""CPU: the host side of gradient clipping / skipping / accumulation and of the resumable training state (ishara_amd/train_state.py):
the numpy references against torch.nn.utils.clip_grad_norm_ and against the oracle's optimizer, the state file's round trip and
refusals, and the refusals of the three new C entry points (all device pointers NULL or made up: a refused call dereferences nothing)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ishara_amd import train_state as TS

N = None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------- grad_stats_reference vs torch
def _three_grads(scale=1.0):
    g = np.random.default_rng(7)
    return [(scale * g.standard_normal(s)).astype(np.float32) for s in ((37,), (64, 13), (5, 1, 301))]


@pytest.mark.parametrize("clip_over_norm", [0.25, 0.999, 1.001, 4.0], ids=lambda v: f"clip{v}xnorm")
def test_grad_stats_reference_equals_clip_grad_norm(clip_over_norm):
    """norm and the clipped gradient (g * coef) against torch on three CPU parameter tensors of different sizes, clip values below and above
    the norm: relative error <= 1e-6, the fp32 rounding of torch's own norm; coef is exactly 1.0 when the norm is under the clip"""
    grads = _three_grads()
    true_norm = float(np.sqrt(sum(float(np.sum(a.astype(np.float64) ** 2)) for a in grads)))
    clip = clip_over_norm * true_norm
    params = [torch.nn.Parameter(torch.zeros(a.shape)) for a in grads]
    for p, a in zip(params, grads):
        p.grad = torch.from_numpy(a.copy())
    tnorm = float(torch.nn.utils.clip_grad_norm_(params, clip))
    st = TS.grad_stats_reference(grads, 1.0, clip)
    assert abs(st["norm"] - tnorm) <= 1e-6 * tnorm, (st["norm"], tnorm)
    assert abs(st["norm"] - true_norm) <= 1e-6 * true_norm
    assert st["nonfinite"] == 0
    if clip_over_norm > 1:
        assert st["coef"] == 1.0
    else:
        assert st["coef"] < 1.0
    for p, a in zip(params, grads):
        want = p.grad.numpy()
        got = a * np.float32(st["coef"])
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()


def test_grad_stats_reference_scale_overflow_and_counts():
    g = np.full(1000, 3e19, np.float32)                     # squares to 9e38, past fp32: the sum has to be taken in fp64
    st = TS.grad_stats_reference(g, 1.0, 0.0)
    want = float(np.float32(3e19)) * np.sqrt(1000.0)
    assert np.isfinite(st["norm"]) and abs(st["norm"] - want) <= 1e-6 * want and st["coef"] == 1.0
    a = _three_grads()[1]
    half = TS.grad_stats_reference(a, 0.5, 0.0)
    full = TS.grad_stats_reference(a, 1.0, 0.0)
    assert half["coef"] == 0.5 and abs(half["norm"] - 0.5 * full["norm"]) <= 1e-6 * full["norm"]
    clipped = TS.grad_stats_reference(a, 0.5, 0.25 * half["norm"])       # coef = grad_scale * clip / norm
    assert abs(clipped["coef"] - 0.5 * 0.25) <= 1e-6
    b = a.reshape(-1).copy()
    b[[0, 5, 17, -1]] = [np.nan, np.inf, -np.inf, np.inf]
    assert TS.grad_stats_reference(b, 1.0, 1.0)["nonfinite"] == 4


# ---------------------------------------------------------------------------------- clipped_step_reference vs the oracle
def test_clipped_step_reference_equals_oracle_bit_for_bit():
    """coef = 1, no skip: 6 steps (across the Lookahead sync at 5) on random fp32 vectors equal oracle.optimizer_step in every bit"""
    from oracle import ishara_oracle as O
    g = np.random.default_rng(3)
    theta0 = g.standard_normal(1000).astype(np.float32)
    ta, tb = theta0.copy(), theta0.copy()
    sa, sb = O.optimizer_init(ta), TS.step_state_init(tb)
    for step in range(6):
        grad = (0.1 * g.standard_normal(1000)).astype(np.float32)
        ta = O.optimizer_step(ta, grad, sa, lr=4e-3)
        tb = TS.clipped_step_reference(tb, grad, sb, lr=4e-3, coef=1.0)
        assert tb.dtype == np.float32
        for x, y in ((ta, tb), (sa.m, sb["m"]), (sa.v, sb["v"]), (sa.slow, sb["slow"])):
            assert np.array_equal(x, y), f"step {step + 1}"
    assert sb["step"] == sa.step == 6 and sb["skipped"] == 0


def test_clipped_step_reference_scales_and_skips():
    from oracle import ishara_oracle as O
    g = np.random.default_rng(4)
    theta = g.standard_normal(64).astype(np.float32)
    grad = g.standard_normal(64).astype(np.float32)
    sa, sb = O.optimizer_init(theta), TS.step_state_init(theta)
    want = O.optimizer_step(theta, grad * np.float32(0.25), sa, lr=1e-2)
    assert np.array_equal(TS.clipped_step_reference(theta, grad, sb, lr=1e-2, coef=0.25), want)
    before = {k: np.copy(v) for k, v in sb.items()}
    bad = grad.copy()
    bad[3] = np.nan
    out = TS.clipped_step_reference(want, bad, sb, lr=1e-2, coef=float("nan"), nonfinite=1, skip_nonfinite=True)
    assert np.array_equal(out, want) and all(np.array_equal(sb[k], before[k]) for k in ("m", "v", "slow"))
    assert sb["step"] == 2 and sb["skipped"] == 1           # the skipped step consumed its iteration number


# ---------------------------------------------------------------------------------- the state file
ENTRIES = [("stem/kernel", (6, 4), 0, True), ("stem/bias", (4,), 24, True), ("bn/moving_mean", (4,), 28, False), ("bn/moving_variance", (4,), 32, False)]


def _state(**kw):
    g = np.random.default_rng(9)
    args = dict(iterations=7, steps=7, step_seed=23774, learning_rate=4e-3, weight_decay=2e-4, apply_weight_decay=True, global_clipnorm=1.5,
                skip_nonfinite=True, accumulate_steps=2, skipped=1)
    args.update(kw)
    return TS.pack_state(ENTRIES, g.standard_normal(36).astype(np.float32), *(g.standard_normal(28).astype(np.float32) for _ in range(3)), **args)


def test_state_round_trip_is_bit_identical(tmp_path):
    st = _state()
    path = TS.save_state_file(str(tmp_path / "run"), st)
    assert path.endswith("run.npz")
    back = TS.load_state_file(str(tmp_path / "run"), ENTRIES)
    for k in TS.ARRAYS:
        assert back[k].dtype == np.float32 and back[k].tobytes() == st[k].tobytes(), k
    assert (back["iterations"], back["steps"], back["step_seed"], back["accumulate_steps"], back["skipped"]) == (7, 7, 23774, 2, 1)
    assert (back["learning_rate"], back["weight_decay"], back["global_clipnorm"]) == (4e-3, 2e-4, 1.5)
    assert back["apply_weight_decay"] is True and back["skip_nonfinite"] is True
    assert TS.unpack_state(_state(global_clipnorm=None), ENTRIES)["global_clipnorm"] is None


def test_state_refusals_have_messages():
    st = _state()
    wrong_shape = [ENTRIES[0], ("stem/bias", (5,), 24, True)] + ENTRIES[2:]
    with pytest.raises(TS.TrainStateError, match=r"wrong shape of 'stem/bias'"):
        TS.unpack_state(st, wrong_shape)
    short = dict(st, opt_v=st["opt_v"][:-1])
    with pytest.raises(TS.TrainStateError, match=r"wrong shape of 'opt_v'"):
        TS.unpack_state(short, ENTRIES)
    missing = {k: v for k, v in st.items() if k != "opt_slow"}
    with pytest.raises(TS.TrainStateError, match=r"missing entry 'opt_slow'"):
        TS.unpack_state(missing, ENTRIES)
    with pytest.raises(TS.TrainStateError, match=r"the model has 'bn/gamma'"):
        TS.unpack_state(st, ENTRIES[:2] + [("bn/gamma", (4,), 28, False)] + ENTRIES[3:])
    with pytest.raises(TS.TrainStateError, match=r"3 parameter entries|4 parameter entries"):
        TS.unpack_state(st, ENTRIES[:3])
    with pytest.raises(TS.TrainStateError, match=r"unknown format version 99"):
        TS.unpack_state(dict(st, format_version=np.int64(99)), ENTRIES)
    with pytest.raises(TS.TrainStateError, match=r"format_version"):
        TS.unpack_state({"params": st["params"]}, ENTRIES)


# ---------------------------------------------------------------------------------- launcher constants
def test_python_constants_are_the_launchers(lib):
    src = open(os.path.join(ROOT, "ishara_amd", "csrc", "grad_ops.hip")).read()
    threads = int(re.search(r"GRAD_THREADS = (\d+);", src).group(1))
    vec = int(re.search(r"GRAD_VEC = (\d+);", src).group(1))
    cap = int(re.search(r"GRAD_GRID_CAP = (\d+);", src).group(1))
    assert (threads * vec, cap) == (TS.GRAD_WG_SPAN, TS.GRAD_GRID_CAP)
    for n in (1, TS.GRAD_WG_SPAN, TS.GRAD_WG_SPAN + 1, TS.GRAD_WG_SPAN * TS.GRAD_GRID_CAP - 1, TS.GRAD_WG_SPAN * TS.GRAD_GRID_CAP + 5, 2 ** 31 - 1):
        assert lib.ishara_grad_stats_workspace_bytes(n) == TS.grad_stats_workspace_bytes(n), n
    assert lib.ishara_grad_stats_workspace_bytes(TS.GRAD_WG_SPAN + 1) == 32 and lib.ishara_grad_stats_workspace_bytes(2 ** 31 - 1) == 16 * TS.GRAD_GRID_CAP


def test_record_struct_matches_header():
    from ishara_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    body = re.search(r"typedef struct ishara_grad_stats \{(.*?)\} ishara_grad_stats;", hdr, re.S).group(1)
    assert re.findall(r"(?:int32_t|float)\s+([a-z_]+);", body) == [f[0] for f in _lib.GradStats._fields_]
    assert C.sizeof(_lib.GradStats) == 16


# ---------------------------------------------------------------------------------- refusals of the C entry points (no GPU, no HIP call)
def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), f"{name}: the error is not the entry point's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


P = lambda a: C.c_void_p(a)      # noqa: E731  made-up addresses


def _stats(lib, g=P(4096), n=100, scale=1.0, clip=1.0, out=P(8192), ws=P(12288)):
    return lib.ishara_gradient_stats(N, g, n, C.c_float(scale), C.c_float(clip), out, ws, N)


def test_gradient_stats_refusals(lib):
    name = "ishara_gradient_stats"
    _refused(lib, _stats(lib, g=N), name, "null g")
    _refused(lib, _stats(lib, out=N), name, "null out")
    _refused(lib, _stats(lib, ws=N), name, "null ws")
    for off in (4, 8, 12):
        _refused(lib, _stats(lib, g=P(4096 + off)), name, "misaligned g", "16-byte")
    _refused(lib, _stats(lib, out=P(8192 + 2)), name, "misaligned out", "4-byte")
    _refused(lib, _stats(lib, ws=P(12288 + 4)), name, "misaligned ws", "8-byte")
    for n in (0, -1, 2 ** 31, 2 ** 40):
        _refused(lib, _stats(lib, n=n), name, f"n={n}", "1..2147483647")
    for scale in (-1.0, float("nan"), float("inf"), -0.5):
        _refused(lib, _stats(lib, scale=scale), name, "grad_scale")
    _refused(lib, _stats(lib, clip=float("nan")), name, "clip_norm", "NaN")
    assert lib.ishara_grad_stats_workspace_bytes(0) < 0
    _refused(lib, -1, "ishara_grad_stats_workspace_bytes", "n=0")
    assert lib.ishara_grad_stats_workspace_bytes(2 ** 31) < 0


def test_gradient_accumulate_refusals(lib):
    name = "ishara_gradient_accumulate"
    call = lambda acc=P(4096), g=P(8192), n=100: lib.ishara_gradient_accumulate(N, acc, g, n, 1, N)      # noqa: E731
    _refused(lib, call(acc=N), name, "null acc")
    _refused(lib, call(g=N), name, "null g")
    _refused(lib, call(acc=P(4096 + 4)), name, "misaligned acc", "16-byte")
    _refused(lib, call(g=P(8192 + 8)), name, "misaligned g", "16-byte")
    _refused(lib, call(g=P(4096)), name, "same buffer")
    for n in (0, -7, 2 ** 31):
        _refused(lib, call(n=n), name, f"n={n}")


def test_optimizer_step_ex_refusals(lib):
    from ishara_amd import make_config
    from ishara_amd.model import Model
    name = "ishara_optimizer_step_ex"
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4), device=None)
    step = lambda h=m._h, grad=N, st=N, skip=0: lib.ishara_optimizer_step_ex(h, C.c_float(1e-3), C.c_float(0.0), grad, st, skip, N)      # noqa: E731
    _refused(lib, step(h=N), name, "null handle")
    _refused(lib, step(grad=P(4096 + 4)), name, "misaligned grad", "16-byte")
    _refused(lib, step(st=P(8192 + 2)), name, "misaligned st")
    _refused(lib, step(skip=1), name, "skip_nonfinite", "null st")
    _refused(lib, step(grad=P(4096), st=P(8192), skip=1), name, "not bound")      # an unbound handle: refused before the launch
    assert lib.ishara_optimizer_iterations(m._h) == 0                             # and no refusal consumed an iteration
    _refused(lib, lib.ishara_optimizer_step(m._h, C.c_float(1e-3), C.c_float(0.0), N), "ishara_optimizer_step", "not bound")


def test_optimizer_options_are_checked():
    from ishara_amd import Optimizer
    o = Optimizer(global_clipnorm=1.0, skip_nonfinite=True, accumulate_steps=4)
    assert o.train_options() == (4, 1.0, True)
    assert Optimizer().train_options() == (1, 0.0, False)
    for bad in (dict(accumulate_steps=0), dict(accumulate_steps=1.5), dict(global_clipnorm=0.0), dict(global_clipnorm=-1.0), dict(global_clipnorm=float("nan"))):
        with pytest.raises(ValueError):
            Optimizer(**bad).train_options()
