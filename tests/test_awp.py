"""CPU: the host side of adversarial weight perturbation (ishara_amd/train_state.py: awp_reference, awp_segments, the optional entries of
the state file), the record's ctypes struct against the header, the refusals of the three C entry points (made-up addresses: a refused
call dereferences nothing), the Optimizer's argument checks and the Model's readers without a step."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import awp_parity as AP
from ishara_amd import _lib, train_state as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = None
P = lambda a: C.c_void_p(a)      # noqa: E731  made-up addresses


# ---------------------------------------------------------------------------------- awp_reference
def _seg_norms(x, seg):
    return np.array([math.sqrt(float(np.sum(x[lo:hi].astype(np.float64) ** 2))) for lo, hi in zip(seg[:-1], seg[1:])])


def test_reference_is_per_tensor_not_global():
    w, g = AP.vectors("A")
    seg = AP.table("A")
    _, scale, stats = TS.awp_reference(w, g, seg, AP.DELTA, AP.EPS)
    want = AP.DELTA / (_seg_norms(g, seg) + AP.EPS)
    assert np.allclose(scale, want, rtol=2e-7, atol=0)
    assert scale.dtype == np.float32 and len(set(scale.tolist())) == len(scale)          # every segment its own factor
    glob = AP.DELTA / (math.sqrt(float(np.sum(g.astype(np.float64) ** 2))) + AP.EPS)
    assert np.all(np.abs(scale / glob - 1) > 1e-3)
    assert stats["perturbed"] == len(scale) and stats["zeroed"] == 0
    assert stats["grad_norm"] == pytest.approx(math.sqrt(float(np.sum(g.astype(np.float64) ** 2))), rel=1e-6)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_reference_moves_every_tensor_by_delta(name):
    """||w_adv - w|| per segment = delta * ||g|| / (||g|| + eps), up to the fp32 rounding of the sum w + d (half an ulp of |w| per element)"""
    w, g = AP.vectors(name)
    seg = AP.table(name)
    w_adv, scale, stats = TS.awp_reference(w, g, seg, AP.DELTA, AP.EPS)
    gn = _seg_norms(g, seg)
    moved = _seg_norms((w_adv.astype(np.float64) - w.astype(np.float64)).astype(np.float32), seg)
    sizes = np.diff(seg)
    slack = np.sqrt(sizes) * 4.0 * np.finfo(np.float32).eps + 1e-6 * AP.DELTA      # |w| < 4 on these vectors
    assert np.all(np.abs(moved - AP.DELTA * gn / (gn + AP.EPS)) <= slack)
    want_delta = math.sqrt(float(np.sum((scale.astype(np.float64) * gn) ** 2)))
    assert stats["delta_norm"] == pytest.approx(want_delta, rel=1e-6)


def test_reference_relative_scales_with_the_weight_norm():
    w, g = AP.vectors("A")
    seg = AP.table("A")
    _, absolute, _ = TS.awp_reference(w, g, seg, AP.DELTA, AP.EPS)
    _, relative, _ = TS.awp_reference(w, g, seg, AP.DELTA, AP.EPS, relative=True)
    assert np.allclose(relative / absolute, _seg_norms(w, seg), rtol=3e-7, atol=0)


def test_reference_update_is_two_fp32_roundings():
    w, g = AP.vectors("A")
    seg = AP.table("A")
    w_adv, scale, _ = TS.awp_reference(w, g, seg, AP.DELTA, AP.EPS)
    per_elem = np.repeat(scale, np.diff(seg))
    assert w_adv.dtype == np.float32 and w_adv.tobytes() == (w + per_elem * g).tobytes()
    fused = (w.astype(np.float64) + per_elem.astype(np.float64) * g.astype(np.float64)).astype(np.float32)      # one rounding: an FMA
    assert 0 < int((fused != w_adv).sum()) < w.size // 4
    assert AP.subnormal_intermediates("A") == 0


def test_reference_zeroed_segments_are_untouched():
    w, g = AP.vectors("A", "nonfinite")
    seg = AP.table("A")
    _, ns, fs, _ = AP.variant_segments(seg)
    w_adv, scale, stats = TS.awp_reference(w, g, seg, AP.DELTA, AP.EPS)
    plain = AP.reference("A")
    assert stats["zeroed"] == 2 and stats["perturbed"] == len(scale) - 2
    for s in range(len(scale)):
        lo, hi = seg[s], seg[s + 1]
        if s in (ns, fs):
            assert scale[s] == 0 and w_adv[lo:hi].tobytes() == w[lo:hi].tobytes()
        else:                                                  # the other segments do not see the NaN and the Inf
            assert scale[s] == plain["scale"][s] and w_adv[lo:hi].tobytes() == plain["w_adv"][lo:hi].tobytes()
    assert math.isfinite(stats["grad_norm"]) and math.isfinite(stats["delta_norm"])
    w2 = w.copy()
    w2[seg[2]] = np.nan                                        # a NaN weight zeroes its segment only under `relative`
    assert TS.awp_reference(w2, AP.vectors("A")[1], seg, AP.DELTA, AP.EPS)[2]["zeroed"] == 0
    _, sc, st = TS.awp_reference(w2, AP.vectors("A")[1], seg, AP.DELTA, AP.EPS, relative=True)
    assert st["zeroed"] == 1 and sc[2] == 0


def test_reference_zero_gradient_and_huge_values():
    seg = AP.table("A")
    zs, _, _, hs = AP.variant_segments(seg)
    w, g = AP.vectors("A", "zero_grad")
    w_adv, scale, stats = TS.awp_reference(w, g, seg, AP.DELTA, AP.EPS)
    assert stats["zeroed"] == 0 and scale[zs] == np.float32(float(np.float32(AP.DELTA)) / float(np.float32(AP.EPS)))
    assert w_adv[seg[zs]:seg[zs + 1]].tobytes() == w[seg[zs]:seg[zs + 1]].tobytes()
    w, g = AP.vectors("A", "huge")
    w_adv, scale, stats = TS.awp_reference(w, g, seg, AP.DELTA, AP.EPS)
    n = int(seg[hs + 1] - seg[hs])
    assert stats["zeroed"] == 0 and scale[hs] == pytest.approx(AP.DELTA / (3e19 * math.sqrt(n)), rel=1e-6)
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(3e19) * np.float32(3e19))   # the squares are past fp32: only an fp64 sum sees them
    assert w_adv[seg[hs]:seg[hs + 1]].tobytes() != w[seg[hs]:seg[hs + 1]].tobytes()


# ---------------------------------------------------------------------------------- awp_segments
def test_segments_cover_the_trainable_prefix_in_entry_order():
    from ishara_amd import make_config
    from ishara_amd.model import Model
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4), device=None)
    seg = TS.awp_segments(m.entries, m.n_train)
    trainable = [(n, int(np.prod(s)), o) for n, s, o, t in m.entries if t]
    assert seg.dtype == np.int64 and len(seg) == len(trainable) + 1
    assert seg[0] == 0 and seg[-1] == m.n_train and np.all(np.diff(seg) >= 1)
    assert [int(o) for o in seg[:-1]] == [o for _, _, o in trainable]            # the layout lists the trainable entries in offset order
    assert [int(d) for d in np.diff(seg)] == [size for _, size, _ in trainable]
    assert np.any(seg % 4 != 0)                                                   # offsets are not 16-byte aligned in general
    assert AP.table("C")[-1] > 0 and np.all(np.diff(AP.table("C")) >= 1)


def test_segments_refuse_a_layout_with_a_hole():
    entries = [("a", (4,), 0, True), ("b", (3,), 5, True), ("bn", (2,), 8, False)]
    with pytest.raises(ValueError, match="do not tile"):
        TS.awp_segments(entries, 8)
    with pytest.raises(ValueError, match="cover"):
        TS.awp_segments([("a", (4,), 0, True), ("bn", (2,), 4, False)], 6)
    assert TS.awp_segments([("b", (3,), 4, True), ("a", (2, 2), 0, True), ("bn", (2,), 7, False)], 7).tolist() == [0, 4, 7]


# ---------------------------------------------------------------------------------- the record and the launcher constants
def test_record_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    body = re.search(r"typedef struct ishara_awp_stats \{(.*?)\} ishara_awp_stats;", hdr, re.S).group(1)
    assert re.findall(r"(?:int64_t|int32_t|float)\s+([a-z_]+);", body) == [f[0] for f in _lib.AwpStats._fields_]
    assert C.sizeof(_lib.AwpStats) == 16
    assert [getattr(_lib.AwpStats, f).offset for f, _ in _lib.AwpStats._fields_] == [0, 4, 8, 12]


def test_launcher_constants():
    src = open(os.path.join(ROOT, "ishara_amd", "csrc", "awp.hip")).read()
    assert int(re.search(r"AWP_CHUNK = (\d+);", src).group(1)) == TS.AWP_CHUNK
    assert int(re.search(r"AWP_GRID_CAP = (\d+);", src).group(1)) == TS.GRAD_GRID_CAP        # a fixed constant, not the CU count
    assert "hipMalloc" not in src and "hipMemset" not in src and "Synchronize" not in src and "atomic" not in src.replace("no float atomics", "")


def test_workspace_bytes(lib):
    ws = lib.ishara_awp_workspace_bytes
    for n, S in ((1, 1), (5, 1), (4096, 1), (4097, 3), (10 ** 6, 107), (2 ** 31 - 1, 1000)):
        bound = -(-n // TS.AWP_CHUNK) + S
        assert ws(n, S) == 8 * (S + 1) + 8 * S + (4 * S + 7) // 8 * 8 + 16 * bound, (n, S)
    for n, S in ((0, 1), (-1, 1), (2 ** 31, 1), (5, 0), (5, 6), (5, -1)):
        assert ws(n, S) == -1 and (lib.ishara_last_error() or b"").decode().startswith("ishara_awp_workspace_bytes:"), (n, S)


# ---------------------------------------------------------------------------------- refusals of the C entry points (no GPU, no HIP call)
def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), f"{name}: the error is not the entry point's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


def test_perturb_refusals(lib):
    name = "ishara_awp_perturb"
    A = dict(w=4096, backup=1 << 20, g=2 << 20, seg_off=3 << 20, scale=4 << 20, rec=5 << 20, ws=6 << 20)

    def call(n=100, S=3, delta=0.2, eps=1e-4, relative=0, **ptr):
        a = {k: P(v) for k, v in A.items()}
        a.update(ptr)
        return lib.ishara_awp_perturb(N, a["w"], a["backup"], a["g"], a["seg_off"], S, n, C.c_float(delta), C.c_float(eps), relative,
                                      a["scale"], a["rec"], a["ws"], N)
    for k in A:
        _refused(lib, call(**{k: N}), name, f"null {k}")
    for off in (4, 8, 12):
        _refused(lib, call(w=P(A["w"] + off)), name, "misaligned w", "16-byte")
        _refused(lib, call(backup=P(A["backup"] + off)), name, "misaligned backup", "16-byte")
    _refused(lib, call(rec=P(A["rec"] + 2)), name, "misaligned rec", "4-byte")
    _refused(lib, call(g=P(A["g"] + 2)), name, "misaligned g", "4-byte")
    _refused(lib, call(scale=P(A["scale"] + 1)), name, "misaligned scale", "4-byte")
    _refused(lib, call(seg_off=P(A["seg_off"] + 4)), name, "misaligned seg_off", "8-byte")
    _refused(lib, call(ws=P(A["ws"] + 4)), name, "misaligned ws", "8-byte")
    _refused(lib, call(backup=P(A["w"])), name, "w and backup overlap")
    _refused(lib, call(backup=P(A["w"] + 400 - 16)), name, "overlap")           # the last 16 bytes of w
    _refused(lib, call(w=P(A["backup"] + 400 - 16)), name, "overlap")
    for n in (0, -1, 2 ** 31, 2 ** 40):
        _refused(lib, call(n=n), name, f"n={n}", "1..2147483647")
    for S in (0, -1, 101):
        _refused(lib, call(S=S), name, f"S={S}", "1..n=100")
    for v in (0.0, -0.2, float("nan"), float("inf"), -float("inf")):
        _refused(lib, call(delta=v), name, "delta")
        _refused(lib, call(eps=v), name, "eps")


def test_restore_refusals(lib):
    name = "ishara_awp_restore"
    call = lambda w=P(4096), backup=P(1 << 20), n=100: lib.ishara_awp_restore(N, w, backup, n, N)      # noqa: E731
    _refused(lib, call(w=N), name, "null w")
    _refused(lib, call(backup=N), name, "null backup")
    _refused(lib, call(w=P(4096 + 8)), name, "misaligned w", "16-byte")
    _refused(lib, call(backup=P((1 << 20) + 4)), name, "misaligned backup", "16-byte")
    _refused(lib, call(backup=P(4096)), name, "overlap")
    _refused(lib, call(backup=P(4096 + 384)), name, "overlap")
    for n in (0, -7, 2 ** 31):
        _refused(lib, call(n=n), name, f"n={n}")


# ---------------------------------------------------------------------------------- Optimizer / Model without a device
def test_optimizer_awp_options_are_checked():
    from ishara_amd import Optimizer
    assert Optimizer().awp_options() == (None, 1e-4, 0, False)
    assert Optimizer().train_options() == (1, 0.0, False) and Optimizer().ema_options() == (False, 0.99, 0, False)      # the existing tuples are what they were
    o = Optimizer(awp_delta=0.2, awp_eps=1e-3, awp_start_step=300, awp_relative=True)
    assert o.awp_options() == (0.2, 1e-3, 300, True)
    assert Optimizer(awp_delta=1, awp_start_step=np.int64(4)).awp_options() == (1.0, 1e-4, 4, False)
    for bad in (dict(awp_delta=0.0), dict(awp_delta=-0.1), dict(awp_delta=float("nan")), dict(awp_delta=float("inf")), dict(awp_delta="0.2"),
                dict(awp_delta=True), dict(awp_delta=1e39), dict(awp_delta=1e-50),                   # inf and 0 as float32, which is what the kernel is handed
                dict(awp_eps=0.0), dict(awp_eps=-1e-4), dict(awp_eps=float("nan")), dict(awp_eps=None), dict(awp_eps=False), dict(awp_eps=1e-60),
                dict(awp_start_step=-1), dict(awp_start_step=2.0), dict(awp_start_step=True), dict(awp_start_step=None)):
        with pytest.raises(ValueError, match="awp_"):
            Optimizer(**dict(dict(awp_delta=0.2), **bad)).awp_options()
    with pytest.raises(ValueError, match="awp_eps"):
        Optimizer(awp_eps=0.0).awp_options()                   # checked also while awp_delta is None


def test_model_without_a_perturbed_step_refuses_its_readers():
    from ishara_amd import Optimizer, make_config
    from ishara_amd.model import Model
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4), device=None)
    m.compile(optimizer=Optimizer(awp_delta=0.2))
    assert m._awp_backup is None and m._awp is None
    for fn in (m.awp_stats, m.awp_scales):
        with pytest.raises(_lib.IsharaError, match="no step has run with adversarial weight perturbation"):
            fn()
    m.optimizer.awp_delta = -1.0                               # the options are plain attributes, checked when a step reads them
    with pytest.raises(ValueError, match="awp_delta"):
        m._awp_begin_step()
    m.optimizer.awp_delta, m.optimizer.awp_start_step = 0.2, 5
    assert m._awp_begin_step() is None and m._awp_backup is None            # not started yet: nothing is allocated
    m.optimizer.awp_delta = None
    assert m._awp_begin_step() is None


# ---------------------------------------------------------------------------------- the state file
ENTRIES = [("stem/kernel", (6, 4), 0, True), ("stem/bias", (4,), 24, True), ("bn/moving_mean", (4,), 28, False), ("bn/moving_variance", (4,), 32, False)]


def _state(**kw):
    g = np.random.default_rng(9)
    args = dict(iterations=7, steps=7, step_seed=23774, learning_rate=4e-3, weight_decay=2e-4, apply_weight_decay=True, global_clipnorm=1.5,
                skip_nonfinite=True, accumulate_steps=2, skipped=1)
    args.update(kw)
    return TS.pack_state(ENTRIES, g.standard_normal(36).astype(np.float32), *(g.standard_normal(28).astype(np.float32) for _ in range(3)), **args)


def test_state_without_awp_has_exactly_the_old_keys():
    assert set(_state()) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS)
    assert set(_state(awp_delta=None, awp_eps=1e-3, awp_start_step=9, awp_relative=True)) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS)
    back = TS.unpack_state(_state(), ENTRIES)
    assert not any(k.startswith("awp_") for k in back) and TS.FORMAT_VERSION == 1
    assert TS.AWP_KEYS == ("awp_delta", "awp_eps", "awp_start_step", "awp_relative")


def test_state_with_awp_round_trips(tmp_path):
    st = _state(awp_delta=0.2, awp_eps=1e-3, awp_start_step=300, awp_relative=True)
    assert set(st) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.AWP_KEYS)
    np.savez(str(tmp_path / "run.npz"), **st)
    with np.load(str(tmp_path / "run.npz"), allow_pickle=False) as z:
        back = TS.unpack_state(z, ENTRIES)
    assert (back["awp_delta"], back["awp_eps"], back["awp_start_step"], back["awp_relative"]) == (0.2, 1e-3, 300, True)
    for k in TS.ARRAYS:
        assert back[k].tobytes() == st[k].tobytes()
    both = _state(awp_delta=0.5, ema_avg=np.zeros(28, np.float32))
    assert set(both) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.EMA_KEYS + TS.AWP_KEYS)
    assert TS.unpack_state(both, ENTRIES)["awp_relative"] is False


def test_state_refuses_wrong_awp_options():
    good = _state(awp_delta=0.2)
    with pytest.raises(TS.TrainStateError, match=r"missing entry 'awp_eps'"):
        TS.unpack_state({k: v for k, v in good.items() if k != "awp_eps"}, ENTRIES)
    for k, v in (("awp_delta", np.float64(0.0)), ("awp_delta", np.float64("nan")), ("awp_eps", np.float64(-1.0)), ("awp_start_step", np.int64(-1))):
        with pytest.raises(TS.TrainStateError, match=r"out of range"):
            TS.unpack_state(dict(good, **{k: v}), ENTRIES)
    with pytest.raises(TS.TrainStateError, match=r"out of range"):
        _state(awp_delta=-0.2)
