"""CPU: the host side of the moving average of the weights (ishara_amd/train_state.py: ema_alpha, ema_reference, the optional entries of
the state file), the record's ctypes struct against the header, the refusals of the two C entry points (made-up addresses: a refused
call dereferences nothing) and the Optimizer's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ishara_amd import _lib, train_state as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = None
P = lambda a: C.c_void_p(a)      # noqa: E731  made-up addresses


# ---------------------------------------------------------------------------------- ema_alpha
@pytest.mark.parametrize("m", [0.0, 0.5, 0.9, 0.99, 0.999, 0.9999])
def test_alpha_without_warmup_is_one_minus_momentum_in_fp64(m):
    want = np.float32(1.0 - np.float64(np.float32(m)))
    for n in (0, 1, 10 ** 6):
        a = TS.ema_alpha(n, m, False)
        assert isinstance(a, np.float32) and a.tobytes() == want.tobytes()


@pytest.mark.parametrize("m", [0.9, 0.99, 0.999])
def test_alpha_with_warmup_follows_the_num_updates_rule(m):
    d = float(np.float32(m))
    for n in (0, 1, 9, 89, 10 ** 6):
        ramp = (1.0 + n) / (10.0 + n)
        want = np.float32(1.0 - min(d, ramp))
        got = TS.ema_alpha(n, m, True)
        assert got.tobytes() == want.tobytes(), (m, n)
        if ramp >= d:
            assert got.tobytes() == TS.ema_alpha(n, m, False).tobytes(), (m, n)
        else:
            assert got > TS.ema_alpha(n, m, False)
    assert TS.ema_alpha(0, m, True) == np.float32(0.9)                  # the first update: d = 1/10
    assert TS.ema_alpha(10 ** 6, m, True) == TS.ema_alpha(0, m, False)


# ---------------------------------------------------------------------------------- ema_reference
def _vectors(n=1000, seed=5):
    g = np.random.default_rng(seed)
    return g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)


def test_reference_update_is_three_fp32_operations():
    avg, theta = _vectors()
    st = TS.ema_state_init()
    out, th = TS.ema_reference(avg, theta, st, 0.9)
    alpha = np.float32(1.0 - np.float64(np.float32(0.9)))
    assert out.dtype == np.float32 and out.tobytes() == (avg + alpha * (theta - avg)).tobytes()
    assert th is theta and st == dict(updates=1, alpha=alpha, overwrote=0)
    close = alpha.astype(np.float64) * theta.astype(np.float64) + (1 - alpha.astype(np.float64)) * avg.astype(np.float64)
    assert np.abs(out - close).max() <= 4 * np.finfo(np.float32).eps * max(np.abs(avg).max(), np.abs(theta).max())


def test_reference_skipped_call_changes_nothing():
    avg, theta = _vectors()
    st = TS.ema_state_init()
    avg, theta = TS.ema_reference(avg, theta, st, 0.9, warmup=True, overwrite_every=1)
    assert st["updates"] == 1 and st["overwrote"] == 1
    a0, t0, alpha0 = avg.copy(), theta.copy(), st["alpha"]
    out, th = TS.ema_reference(avg, theta + 1, st, 0.9, warmup=True, overwrite_every=1, nonfinite=3, skip_nonfinite=True)
    assert out.tobytes() == a0.tobytes() and th.tobytes() == (t0 + 1).tobytes()
    assert st == dict(updates=1, alpha=alpha0, overwrote=0)
    out, _ = TS.ema_reference(avg, theta + 1, st, 0.9, warmup=True, nonfinite=3, skip_nonfinite=False)       # the guard is off: it updates
    assert st["updates"] == 2 and out.tobytes() != a0.tobytes()


def test_reference_overwrites_every_second_update():
    avg, theta0 = _vectors()
    st = TS.ema_state_init()
    g = np.random.default_rng(6)
    for k in range(1, 5):
        theta_in = theta0 + g.standard_normal(theta0.size).astype(np.float32)
        avg, theta = TS.ema_reference(avg, theta_in, st, 0.75, overwrite_every=2)
        assert st["updates"] == k and st["overwrote"] == (1 if k % 2 == 0 else 0)
        if k % 2 == 0:
            assert theta.tobytes() == avg.tobytes() and theta is not avg
        else:
            assert theta is theta_in


# ---------------------------------------------------------------------------------- the state file
ENTRIES = [("stem/kernel", (6, 4), 0, True), ("stem/bias", (4,), 24, True), ("bn/moving_mean", (4,), 28, False), ("bn/moving_variance", (4,), 32, False)]


def _state(**kw):
    g = np.random.default_rng(9)
    args = dict(iterations=7, steps=7, step_seed=23774, learning_rate=4e-3, weight_decay=2e-4, apply_weight_decay=True, global_clipnorm=1.5,
                skip_nonfinite=True, accumulate_steps=2, skipped=1)
    args.update(kw)
    return TS.pack_state(ENTRIES, g.standard_normal(36).astype(np.float32), *(g.standard_normal(28).astype(np.float32) for _ in range(3)), **args)


def _avg():
    return np.random.default_rng(10).standard_normal(28).astype(np.float32)


def test_state_without_the_average_has_exactly_the_old_keys():
    assert set(_state()) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS)
    assert TS.FORMAT_VERSION == 1
    back = TS.unpack_state(_state(), ENTRIES)                  # a version-1 file without the keys still validates
    assert not any(k.startswith("ema_") or k == "use_ema" for k in back)


def test_state_with_the_average_round_trips(tmp_path):
    st = _state(ema_avg=_avg(), ema_updates=41, use_ema=True, ema_momentum=0.999, ema_warmup=True, ema_overwrite_frequency=100)
    assert set(st) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.EMA_KEYS)
    np.savez(str(tmp_path / "run.npz"), **st)
    with np.load(str(tmp_path / "run.npz"), allow_pickle=False) as z:
        back = TS.unpack_state(z, ENTRIES)
    assert back["ema_avg"].dtype == np.float32 and back["ema_avg"].tobytes() == _avg().tobytes()
    assert (back["ema_updates"], back["use_ema"], back["ema_momentum"], back["ema_warmup"], back["ema_overwrite_frequency"]) == (41, True, 0.999, True, 100)
    for k in TS.ARRAYS:
        assert back[k].tobytes() == st[k].tobytes()
    off = TS.unpack_state(_state(ema_avg=_avg(), ema_overwrite_frequency=None, use_ema=False), ENTRIES)
    assert off["ema_overwrite_frequency"] is None and off["use_ema"] is False and off["ema_updates"] == 0


def test_state_refuses_a_wrong_average():
    with pytest.raises(TS.TrainStateError, match=r"wrong shape of 'ema_avg'.*float32\(27,\).*expected float32\(28,\)"):
        _state(ema_avg=_avg()[:-1])
    with pytest.raises(TS.TrainStateError, match=r"wrong shape of 'ema_avg'.*float64"):
        _state(ema_avg=_avg().astype(np.float64))
    good = _state(ema_avg=_avg())
    with pytest.raises(TS.TrainStateError, match=r"wrong shape of 'ema_avg'"):
        TS.unpack_state(dict(good, ema_avg=np.zeros(36, np.float32)), ENTRIES)       # the size of params, not of the trainable prefix
    with pytest.raises(TS.TrainStateError, match=r"missing entry 'ema_updates'"):
        TS.unpack_state({k: v for k, v in good.items() if k != "ema_updates"}, ENTRIES)
    with pytest.raises(TS.TrainStateError, match=r"out of range"):
        TS.unpack_state(dict(good, ema_momentum=np.float64(1.0)), ENTRIES)


# ---------------------------------------------------------------------------------- the record and the launcher constants
def test_record_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    body = re.search(r"typedef struct ishara_ema_state \{(.*?)\} ishara_ema_state;", hdr, re.S).group(1)
    assert re.findall(r"(?:int64_t|int32_t|float)\s+([a-z_]+);", body) == [f[0] for f in _lib.EmaState._fields_]
    assert C.sizeof(_lib.EmaState) == 16 and _lib.EmaState.alpha.offset == 8 and _lib.EmaState.overwrote.offset == 12


def test_launcher_constants_are_grad_ops():
    src = open(os.path.join(ROOT, "ishara_amd", "csrc", "weight_avg.hip")).read()
    threads = int(re.search(r"WAVG_THREADS = (\d+);", src).group(1))
    vec = int(re.search(r"WAVG_VEC = (\d+);", src).group(1))
    cap = int(re.search(r"WAVG_GRID_CAP = (\d+);", src).group(1))
    assert (threads, threads * vec, cap) == (256, TS.GRAD_WG_SPAN, TS.GRAD_GRID_CAP)


# ---------------------------------------------------------------------------------- refusals of the C entry points (no GPU, no HIP call)
def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), f"{name}: the error is not the entry point's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


def test_weight_average_refusals(lib):
    name = "ishara_weight_average"

    def call(avg=P(4096), theta=P(1 << 20), n=100, momentum=0.9, every=0, rec=P(8192 << 10), st=N, skip=0):
        return lib.ishara_weight_average(N, avg, theta, n, C.c_float(momentum), 0, every, rec, st, skip, N)
    _refused(lib, call(avg=N), name, "null avg")
    _refused(lib, call(theta=N), name, "null theta")
    _refused(lib, call(rec=N), name, "null rec")
    for off in (4, 8, 12):
        _refused(lib, call(avg=P(4096 + off)), name, "misaligned avg", "16-byte")
        _refused(lib, call(theta=P((1 << 20) + off)), name, "misaligned theta", "16-byte")
    _refused(lib, call(rec=P((8192 << 10) + 4)), name, "misaligned rec", "8-byte")
    for n in (0, -1, 2 ** 31, 2 ** 40):
        _refused(lib, call(n=n), name, f"n={n}", "1..2147483647")
    _refused(lib, call(theta=P(4096)), name, "overlap")
    _refused(lib, call(theta=P(4096 + 400 - 16)), name, "overlap")          # the last 16 bytes of avg
    _refused(lib, call(avg=P(4096 + 400 - 16), theta=P(4096)), name, "overlap")
    for m in (1.0, -0.1, 1.5, float("nan"), float("inf")):
        _refused(lib, call(momentum=m), name, "momentum")
    _refused(lib, call(every=-1), name, "overwrite_every")
    _refused(lib, call(skip=1), name, "skip_nonfinite", "null st")


def test_weight_swap_refusals(lib):
    name = "ishara_weight_swap"
    call = lambda a=P(4096), b=P(1 << 20), n=100: lib.ishara_weight_swap(N, a, b, n, N)      # noqa: E731
    _refused(lib, call(a=N), name, "null a")
    _refused(lib, call(b=N), name, "null b")
    _refused(lib, call(a=P(4096 + 8)), name, "misaligned a", "16-byte")
    _refused(lib, call(b=P((1 << 20) + 4)), name, "misaligned b", "16-byte")
    _refused(lib, call(b=P(4096)), name, "overlap")
    _refused(lib, call(b=P(4096 + 384)), name, "overlap")
    for n in (0, -7, 2 ** 31):
        _refused(lib, call(n=n), name, f"n={n}")


# ---------------------------------------------------------------------------------- Optimizer / Model without a device
def test_optimizer_ema_options_are_checked():
    from ishara_amd import Optimizer
    assert Optimizer().ema_options() == (False, 0.99, 0, False)
    assert Optimizer().train_options() == (1, 0.0, False)                       # the existing tuple is what it was
    o = Optimizer(use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=100, ema_warmup=True, global_clipnorm=1.0)
    assert o.ema_options() == (True, 0.9, 100, True) and o.train_options() == (1, 1.0, False)
    for bad in (dict(ema_momentum=1.0), dict(ema_momentum=-0.1), dict(ema_momentum=float("nan")), dict(ema_momentum="0.9"), dict(ema_momentum=None),
                dict(ema_momentum=0.999999999),               # 1.0 as float32, which is what the kernel is handed
                dict(ema_overwrite_frequency=0), dict(ema_overwrite_frequency=-1), dict(ema_overwrite_frequency=2.5), dict(ema_overwrite_frequency=True)):
        with pytest.raises(ValueError):
            Optimizer(use_ema=True, **bad).ema_options()


def test_model_without_an_average_refuses_its_readers():
    from ishara_amd import Optimizer, make_config
    from ishara_amd.model import Model
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4), device=None)
    m.compile(optimizer=Optimizer(use_ema=True))
    assert m._ema_avg is None and m._ema_rec is None
    for fn in (m.ema_weights, m.ema_state, m.finalize_ema, lambda: m.averaged_weights().__enter__()):
        with pytest.raises(_lib.IsharaError, match="no moving average"):
            fn()
    m.optimizer.ema_momentum = 1.0                             # the options are plain attributes, checked when a step reads them
    with pytest.raises(ValueError, match="ema_momentum"):
        m.optimizer.ema_options()
    with pytest.raises(ValueError, match="ema_momentum"):
        m._ema_begin_step()
