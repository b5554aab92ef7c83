"""CPU: knowledge distillation's host side (ishara_amd/kd.py, train_state.py, model.py) and the refusals of its two entry points, which come
before any HIP call.

  the fp64 definition against torch.autograd of tau^2 * F.kl_div(log_softmax(z / tau), softmax(u / tau)), with lengths and both modes
  the float32 twin of the kernel (tests/kd_parity.py) within the bound on every case; K_HOST and K_HOST_KL are what the twin measures
  Optimizer(kd_*) option checking, Model.set_teacher's checks, nothing allocated without an active step
  the state file's optional key `kd`
  the header declares and the library exports the two symbols; every refusal of ishara_kd_grad and of ishara_loss_backward_kd"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kd_parity as P
from ishara_amd import kd
from ishara_amd import train_state as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p
N_ = None


# ---------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("tau", [1.0, 2.0, 4.0, 0.5])
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_reference_equals_autograd_of_the_tempered_kl(tau, mode):
    import torch
    import torch.nn.functional as F
    g = np.random.default_rng(260)
    B, T, Cn = 3, 7, 6
    z, u = g.standard_normal((B, T, Cn)) * 2, g.standard_normal((B, T, Cn)) * 2
    fl = np.array([7, 3, 0])
    lam = 0.7
    ref = kd.kd_reference(z, u, 1.0 / tau, mode, fl, lam * tau / B)          # tau in {1, 2, 4, 0.5}: 1 / tau and lam * tau / B as float32 ...
    gs = float(np.float32(lam * tau / B))                                    # ... the reference takes grad_scale at its float32 value
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    kl = F.kl_div(F.log_softmax(zt / tau, -1), F.softmax(torch.tensor(u) / tau, -1), reduction="none").sum(-1)          # [B, T]
    inside = torch.tensor(np.arange(T)[None, :] < fl[:, None])
    w = torch.tensor([1.0 / max(int(n), 1) if mode == "mean" else 1.0 for n in fl], dtype=torch.float64)
    per_clip = (kl * inside).sum(1) * w
    (gs * tau * per_clip.sum()).backward()                                   # grad_scale * tau * sum_b w_b * sum_t KL_t
    assert np.allclose(ref["grad"], zt.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert np.allclose(ref["kl_frame"], (kl * inside).detach().numpy(), rtol=1e-12, atol=1e-15)
    assert np.allclose(ref["kl_clip"], per_clip.detach().numpy(), rtol=1e-12, atol=1e-15)
    assert (ref["grad"][1, 3:] == 0).all() and (ref["grad"][2] == 0).all() and list(ref["frames"]) == [7, 3, 0]


def test_reference_does_not_read_rows_past_a_clips_end_and_refuses_bad_arguments():
    z = np.zeros((2, 4, 3))
    z[0, 2:] = np.nan
    ref = kd.kd_reference(z, z, 1.0, "mean", [2, 9])
    assert np.isfinite(ref["grad"]).all() and (ref["kl_clip"] == 0).all() and list(ref["frames"]) == [2, 0]
    with pytest.raises(ValueError, match="mode"):
        kd.kd_reference(z, z, mode="max")
    with pytest.raises(ValueError, match="one shape"):
        kd.kd_reference(z, z[:, :3])
    with pytest.raises(ValueError, match="frame_lengths"):
        kd.kd_reference(z, z, frame_lengths=[1, 2, 3])


def test_the_twin_passes_every_case_and_the_constants_are_what_was_measured():
    kg, kk = P.measure_k_host()
    print(f"K_HOST measured {kg:.3f}, recorded {P.K_HOST}, K = {P.K}; K_HOST_KL measured {kk:.3f}, recorded {P.K_HOST_KL}, K_KL = {P.K_KL}")
    # numpy's float32 exp / log differ by an ulp between its SIMD builds, which moves the worst case a little: the recorded constants must
    # stay what such a measurement gives, not become free parameters
    assert kg <= P.K_HOST <= 2 * kg and kk <= P.K_HOST_KL <= 2 * kk, "a recorded constant is not what the fp32 twin measures on this host"
    assert P.K == 4 * P.K_HOST and P.K_KL == 4 * P.K_HOST_KL
    for c in P.cases():
        t = P.twin(c)
        o = P.old_rows(c)
        ta = P.twin(c, old=o)
        assert P.compare_grad(c, t["dlogits"]) <= 1 and P.compare_kl(c, t["kl_frame"]) <= 1 and P.compare_grad(c, ta["dlogits"], old=o) <= 1, c["name"]
        assert np.array_equal(t["dlb"], P.dlb_of(t["dlogits"])) and np.array_equal(ta["dlb"], P.dlb_of(ta["dlogits"])), c["name"]
        assert np.array_equal(t["kl_clip"], P.clip_sum(t["kl_frame"], c)), c["name"]
        if c["kind"] == "same":
            assert not t["dlogits"].any() and not t["kl_frame"].any(), c["name"]


def test_case_table_holds_what_the_issue_asks_for():
    cs = P.cases()
    assert {c["C"] for c in cs} == {2, 5, 59, 60, 64} and {c["T"] for c in cs} >= {1, 15, 16, 17, 33} and {c["B"] for c in cs} == {1, 2, 3}
    assert {c["inv_temp"] for c in cs} == {1.0, 0.5, 0.25, 2.0} and {c["mode"] for c in cs} == {0, 1}
    assert any(c["kind"] == "big" and np.nanmax(np.abs(c["logits"])) == 80 and np.nanmax(np.abs(c["teacher"])) == 80 for c in cs)
    lp = next(c for c in cs if c["kind"] == "logprob" and c["fkind"] != "mix")
    assert np.allclose(np.exp(lp["teacher"].astype(np.float64)).sum(-1), 1.0, atol=1e-5)
    seen = set()
    for c in cs:
        if c["fkind"] == "mix":
            T = c["T"]
            seen |= {("0" if v == 0 else "1" if v == 1 else "T-1" if v == T - 1 else "T" if v == T else "T+1" if v == T + 1 else "neg") for v in c["frame_len"]}
    assert seen >= {"0", "1", "T-1", "T", "T+1", "neg"}


def test_bf16_helper_rounds_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -8, -0.0, 0.0], np.float32)
    assert list(P.bf16_rne(x)) == [0x3F80, 0x3F80, 0x3F81, 0x3F82, 0x8000, 0x0000]


# ---------------------------------------------------------------------------------- options, teacher, allocation
def test_optimizer_kd_options_are_checked():
    from ishara_amd import Optimizer
    assert Optimizer().kd_options() == dict(kd_weight=0.0, kd_temperature=2.0, kd_ctc_weight=1.0, kd_normalise=True, kd_start_step=0)
    assert kd.OPTION_NAMES == tuple(Optimizer().kd_options())
    o = Optimizer(kd_weight=0.5, kd_temperature=4, kd_ctc_weight=0, kd_normalise=False, kd_start_step=np.int64(9))
    assert o.kd_options() == dict(kd_weight=0.5, kd_temperature=4.0, kd_ctc_weight=0.0, kd_normalise=False, kd_start_step=9)
    for bad in (dict(kd_weight=-1), dict(kd_weight=float("nan")), dict(kd_weight=True), dict(kd_weight="1"), dict(kd_temperature=0), dict(kd_temperature=float("inf")),
                dict(kd_temperature=1e-60), dict(kd_ctc_weight=-0.1), dict(kd_normalise=1), dict(kd_start_step=-1), dict(kd_start_step=1.5), dict(kd_start_step=True)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            Optimizer(**bad).kd_options()
    with pytest.raises(TypeError):
        kd.check_options(kd_depth=2)


def test_model_without_such_a_step_allocates_nothing_and_refuses_its_reader():
    from ishara_amd import Optimizer, _lib, make_config
    from ishara_amd.model import Model
    kw = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4)
    m = Model(make_config(**kw), device=None)
    assert m._kd is None and m._teacher is None and m._kd_begin_step() is None
    m.compile(optimizer=Optimizer(kd_weight=1.0, kd_start_step=5))
    assert m._kd_begin_step() is None and m._kd is None                      # not started yet: nothing is allocated
    with pytest.raises(_lib.IsharaError, match="no step has run with distillation"):
        m.kd_stats()
    m.optimizer.kd_weight = -1.0                                # the options are plain attributes, checked when a step reads them
    with pytest.raises(ValueError, match="kd_weight"):
        m._kd_begin_step()
    # set_teacher's checks need no device
    same = Model(make_config(**dict(kw, dim=128)), device=None)
    assert m.set_teacher(same) is m and m._teacher[0] == "models" and m._teacher[2] is None
    m.set_teacher([same, same], weights=[1, 3], mode="linear")
    assert np.allclose(m._teacher[2], [0.25, 0.75]) and m._teacher[3] == "linear"
    m.set_teacher(lambda x, fl: None)
    assert m._teacher[0] == "callable"
    assert m.set_teacher(None)._teacher is None
    with pytest.raises(ValueError, match="same"):
        m.set_teacher(Model(make_config(**dict(kw, input_shape=(48, 36))), device=None))
    for bad, word in ((dict(teacher=3), "teacher must be"), (dict(teacher=[same], mode="max"), "mode"), (dict(teacher=[same, same], weights=[1]), "weights"),
                      (dict(teacher=[]), "0 teacher models"), (dict(teacher=len, weights=[1]), "weights belong")):
        with pytest.raises(ValueError, match=word):
            m.set_teacher(**bad)


# ---------------------------------------------------------------------------------- the state file
ENTRIES = [("stem/kernel", (6, 4), 0, True), ("stem/bias", (4,), 24, True), ("bn/moving_mean", (4,), 28, False), ("bn/moving_variance", (4,), 32, False)]
OPTS = dict(kd_weight=0.5, kd_temperature=4.0, kd_ctc_weight=0.25, kd_normalise=False, kd_start_step=300)


def _state(**kw):
    g = np.random.default_rng(9)
    args = dict(iterations=7, steps=7, step_seed=23774, learning_rate=4e-3, weight_decay=2e-4, apply_weight_decay=True, global_clipnorm=1.5,
                skip_nonfinite=True, accumulate_steps=2, skipped=1)
    args.update(kw)
    return TS.pack_state(ENTRIES, g.standard_normal(36).astype(np.float32), *(g.standard_normal(28).astype(np.float32) for _ in range(3)), **args)


def test_state_without_kd_has_exactly_the_old_keys():
    assert set(_state()) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS) and TS.FORMAT_VERSION == 1
    assert "kd" not in TS.unpack_state(_state(), ENTRIES) and TS.KD_KEYS == ("kd",)


def test_state_with_kd_round_trips_as_one_key(tmp_path):
    st = _state(kd=OPTS)
    assert set(st) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.KD_KEYS)
    np.savez(str(tmp_path / "run.npz"), **st)
    with np.load(str(tmp_path / "run.npz"), allow_pickle=False) as z:
        back = TS.unpack_state(z, ENTRIES)
    assert back["kd"] == OPTS
    for k in TS.ARRAYS:
        assert back[k].tobytes() == st[k].tobytes()
    both = TS.unpack_state(_state(kd=OPTS, mwer=dict(mwer_nbest=4)), ENTRIES)
    assert both["kd"] == OPTS and both["mwer"]["mwer_nbest"] == 4


def test_state_refuses_wrong_kd_options():
    good = _state(kd=OPTS)
    for text in ('{"kd_weight": -1}', '{"kd_weight": 1, "kd_depth": 2}', "[4]", '{"kd_temperature": 0}'):
        with pytest.raises(TS.TrainStateError, match="'kd'"):
            TS.unpack_state(dict(good, kd=np.array(text, dtype=np.str_)), ENTRIES)
    with pytest.raises(ValueError, match="kd_weight"):
        _state(kd=dict(OPTS, kd_weight=-2))


# ---------------------------------------------------------------------------------- the C ABI: symbols and refusals (no HIP call is reached)
def test_new_symbols_are_declared_in_the_header_and_exported(lib):
    from ishara_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    for name in ("ishara_kd_grad", "ishara_loss_backward_kd"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for struct, cls in (("ishara_kd_stage", _lib.KdStage), ("ishara_nbest_stage", _lib.NbestStage)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n.strip() for decl in re.findall(r"(?:const )?(?:float|int32_t|void)\*? ([A-Za-z_, ]+);", body) for n in decl.split(",")]
        assert fields == [f[0] for f in cls._fields_], struct


def test_source_keeps_the_launch_conditions():
    src = open(os.path.join(ROOT, "ishara_amd", "csrc", "kd_grad.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    for word in ("atomic", "hipMalloc", "hipMemset", "hipMemcpy", "Synchronize"):
        assert word not in code, word
    assert code.count("#pragma clang fp contract(off)") >= 5


def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), f"{name}: the error is not the entry point's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


P0 = dict(logits=1 << 20, teacher=2 << 20, dlogits=3 << 20)
B0, T0, C0 = 2, 16, 8


def kd_call(lib, B=B0, T=T0, Cn=C0, inv_temp=1.0, mode=0, grad_scale=1.0, accumulate=0, frame_len=N_, dlb=N_, kl_frame=N_, kl_clip=N_, **ptr):
    a = {k: A(v) for k, v in P0.items()}
    a.update(ptr)
    return lib.ishara_kd_grad(N_, a["logits"], a["teacher"], B, T, Cn, C.c_float(inv_temp), mode, frame_len, C.c_float(grad_scale), a["dlogits"], accumulate, dlb,
                              kl_frame, kl_clip, N_)


def check_kd_grad_refusals(lib):
    """every refusal of ishara_kd_grad, on pointers that are never dereferenced (tests/test_kd_gpu.py runs it on a GPU as well)"""
    name = "ishara_kd_grad"
    for kw, word in ((dict(Cn=1), "C=1"), (dict(Cn=65), "C=65"), (dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(B=-1), "B=-1"), (dict(B=65536), "B=65536"),
                     (dict(mode=2), "mode 2"), (dict(mode=-1), "mode -1"), (dict(accumulate=2), "accumulate=2"), (dict(accumulate=-1), "accumulate=-1"),
                     (dict(inv_temp=0.0), "inv_temp"), (dict(inv_temp=-1.0), "inv_temp"), (dict(inv_temp=float("inf")), "inv_temp"),
                     (dict(inv_temp=float("nan")), "inv_temp"), (dict(grad_scale=float("inf")), "grad_scale"), (dict(grad_scale=float("nan")), "grad_scale"),
                     (dict(kl_clip=A(5 << 20)), "kl_clip needs kl_frame")):
        _refused(lib, kd_call(lib, **kw), name, word)
    for k in P0:
        _refused(lib, kd_call(lib, **{k: N_}), name, "null " + k)
        _refused(lib, kd_call(lib, **{k: A(P0[k] + 2)}), name, "misaligned")
    for k in ("frame_len", "dlb", "kl_frame"):
        _refused(lib, kd_call(lib, **{k: A((7 << 20) + 1)}), name, "misaligned")
    _refused(lib, kd_call(lib, kl_frame=A(7 << 20), kl_clip=A((8 << 20) + 2)), name, "misaligned")
    nin = B0 * T0 * C0 * 4
    _refused(lib, kd_call(lib, dlogits=A(P0["logits"])), name, "dlogits overlaps logits")
    _refused(lib, kd_call(lib, dlogits=A(P0["teacher"] + nin - 4)), name, "dlogits overlaps teacher")
    _refused(lib, kd_call(lib, dlogits=A(P0["logits"] - nin + 4)), name, "dlogits overlaps logits")
    _refused(lib, kd_call(lib, dlb=A(P0["dlogits"] + 4)), name, "overlaps")
    _refused(lib, kd_call(lib, kl_frame=A(P0["teacher"])), name, "kl_frame overlaps teacher")
    _refused(lib, kd_call(lib, kl_frame=A(7 << 20), kl_clip=A((7 << 20) + B0 * T0 * 4 - 4)), name, "overlaps")
    assert kd_call(lib, B=0) == 0                               # a no-op: nothing is launched, nothing is dereferenced
    assert kd_call(lib, B=0, logits=N_, teacher=N_, dlogits=N_) == 0


def test_kd_grad_refusals(lib):
    check_kd_grad_refusals(lib)


def test_loss_backward_kd_refuses_before_any_launch(lib):
    from ishara_amd import _lib, make_config
    from ishara_amd.model import Model
    name = "ishara_loss_backward_kd"
    stage = _lib.KdStage(2 << 20, 1.0, 0, 1.0, None, None)
    rc = lib.ishara_loss_backward_kd(N_, A(1 << 20), A(3 << 20), 2, N_, N_, C.c_float(1.0), N_, C.byref(stage), N_, N_)
    _refused(lib, rc, name, "null model")
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4), device=None)       # a handle without buffers
    call = lambda st, nb=N_, B=2: lib.ishara_loss_backward_kd(m._h, A(1 << 20), A(3 << 20), B, N_, N_, C.c_float(1.0), N_, C.byref(st), nb, N_)
    _refused(lib, call(stage, B=0), name, "B=0")
    for st, word in ((_lib.KdStage(2 << 20, 0.0, 0, 1.0, None, None), "inv_temp"), (_lib.KdStage(2 << 20, 1.0, 3, 1.0, None, None), "mode 3"),
                     (_lib.KdStage(2 << 20, 1.0, 0, float("inf"), None, None), "kd_scale"), (_lib.KdStage(2 << 20, 1.0, 0, 1.0, None, 5 << 20), "kl_clip needs kl_frame"),
                     (_lib.KdStage(None, 1.0, 0, 1.0, None, None), "null teacher"), (_lib.KdStage((2 << 20) + 2, 1.0, 0, 1.0, None, None), "null dlogits")):
        _refused(lib, call(st), name, word)                     # the last one: an unbound model has no dlogits, and says so before the alignment
    nb = _lib.NbestStage(4 << 20, 5 << 20, 0, 16, 16, 6 << 20, 1.0, 7 << 20)
    _refused(lib, call(stage, C.byref(nb)), name, "N=0")          # the n-best stage's own refusals come first
