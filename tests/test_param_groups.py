"""CPU: the host side of the optimizer's parameter groups (ishara_amd/train_state.py: the checks, the resolution of patterns over entry
names, the device rows, no_decay_groups, param_groups_reference, mask_reference, the optional state entry), the row's struct against the
header, the parity cases' own premises, and the Model's change-by-value detector without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import param_groups_parity as PG
from ishara_amd import _lib, train_state as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    from ishara_amd import make_config
    from ishara_amd.model import Model
    return Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4), device=None)


def _trainable(m):
    return [n for _, n in sorted((o, n) for n, _, o, t in m.entries if t)]


# ---------------------------------------------------------------------------------- resolution
def test_first_match_wins_and_unmatched_entries_keep_the_defaults(model):
    names = _trainable(model)
    kernels = [n for n in names if n.endswith("/kernel")]
    assert kernels and len(kernels) < len(names)
    first = kernels[0]
    groups = [dict(match=first, lr_scale=4.0), dict(match=["*/kernel", first], weight_decay_scale=0.5, trainable=False)]
    res = TS.resolve_param_groups(model.entries, groups)
    assert list(res) == names                                      # offset order, trainable entries only
    assert res[first] == dict(lr_scale=4.0, weight_decay_scale=1.0, trainable=True)
    for n in names:
        if n in kernels[1:]:
            assert res[n] == dict(lr_scale=1.0, weight_decay_scale=0.5, trainable=False)
        elif n != first:
            assert res[n] == dict(lr_scale=1.0, weight_decay_scale=1.0, trainable=True)
    assert TS.resolve_param_groups(model.entries, None) == {n: dict(lr_scale=1.0, weight_decay_scale=1.0, trainable=True) for n in names}
    # fnmatchcase: the case of a pattern counts
    with pytest.raises(ValueError, match=re.escape(repr(first.upper()))):
        TS.resolve_param_groups(model.entries, [dict(match=first.upper())])


def test_a_pattern_without_a_trainable_entry_raises_and_is_named(model):
    moving = [n for n, _, _, t in model.entries if not t]
    assert moving and all(n.endswith(("moving_mean", "moving_variance")) for n in moving)
    for pat in ("*moving_mean", "*/moving_variance", moving[0], "no/such/tensor", "*/kernle"):
        with pytest.raises(ValueError, match=re.escape(repr(pat))):
            TS.resolve_param_groups(model.entries, [dict(match="*"), dict(match=["*/bias", pat])])


def test_rows_follow_the_segment_table(model):
    names = _trainable(model)
    groups = [dict(match=names[1], trainable=False), dict(match=names[-1], lr_scale=0.25, weight_decay_scale=0.0)]
    seg, rows = TS.param_group_rows(model.entries, model.n_train, groups)
    assert np.array_equal(seg, TS.awp_segments(model.entries, model.n_train)) and rows.dtype == TS.PARAM_GROUP_DTYPE and len(rows) == len(names)
    assert rows[1].tolist() == (1.0, 1.0, 1, 0) and rows[-1].tolist() == (0.25, 0.0, 0, 0) and rows[0].tolist() == (1.0, 1.0, 0, 0)
    assert int((rows["frozen"] != 0).sum()) == 1 and not rows["reserved"].any()


# ---------------------------------------------------------------------------------- validation
def test_groups_are_checked():
    from ishara_amd import Optimizer
    assert Optimizer().group_options() is None and Optimizer().param_groups is None
    o = Optimizer(param_groups=[{"match": "*/bias"}, {"match": ["a", "b"], "lr_scale": 2, "weight_decay_scale": np.float32(0.5), "trainable": False}])
    assert o.group_options() == [dict(match=["*/bias"], lr_scale=1.0, weight_decay_scale=1.0, trainable=True),
                                 dict(match=["a", "b"], lr_scale=2.0, weight_decay_scale=0.5, trainable=False)]
    assert Optimizer().awp_options() == (None, 1e-4, 0, False) and Optimizer().train_options() == (1, 0.0, False)      # the other tuples are what they were
    for bad in ("*/bias", {"match": "*"}, [["*"]], [{}], [{"match": "*", "lr": 1.0}], [{"match": ""}], [{"match": []}], [{"match": [1]}], [{"match": None}],
                [{"match": "*", "lr_scale": -1.0}], [{"match": "*", "lr_scale": float("nan")}], [{"match": "*", "lr_scale": float("inf")}],
                [{"match": "*", "lr_scale": 1e39}], [{"match": "*", "lr_scale": "1"}], [{"match": "*", "lr_scale": True}], [{"match": "*", "lr_scale": None}],
                [{"match": "*", "weight_decay_scale": -0.5}], [{"match": "*", "weight_decay_scale": float("nan")}], [{"match": "*", "weight_decay_scale": 1e39}],
                [{"match": "*", "trainable": 0}], [{"match": "*", "trainable": None}]):
        with pytest.raises(ValueError, match="param_groups"):
            Optimizer(param_groups=bad).group_options()
    assert Optimizer(param_groups=[{"match": "*", "lr_scale": 0, "weight_decay_scale": 0.0}]).group_options()[0]["lr_scale"] == 0.0      # 0 is allowed


def test_row_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    body = re.search(r"typedef struct ishara_param_group \{(.*?)\} ishara_param_group;", hdr, re.S).group(1)
    fields = re.findall(r"(?:int64_t|int32_t|float)\s+([a-z_]+);", body)
    assert fields == [f[0] for f in _lib.ParamGroup._fields_] == list(TS.PARAM_GROUP_DTYPE.names)
    assert C.sizeof(_lib.ParamGroup) == 16 == TS.PARAM_GROUP_DTYPE.itemsize
    assert [getattr(_lib.ParamGroup, f).offset for f, _ in _lib.ParamGroup._fields_] == [0, 4, 8, 12] == [TS.PARAM_GROUP_DTYPE.fields[f][1] for f in fields]
    for name in ("ishara_param_groups_workspace_bytes", "ishara_optimizer_step_groups", "ishara_gradient_mask_groups", "ishara_optimizer_op_step",
                 "ishara_optimizer_op_step_groups"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\(", hdr), name


def test_no_decay_groups_names_exactly_the_one_dimensional_entries(model):
    (g,) = TS.no_decay_groups(model.entries)
    assert g["weight_decay_scale"] == 0.0 and set(g) == {"match", "weight_decay_scale"}
    want = {n for n, s, _, t in model.entries if t and len(s) <= 1}
    assert set(g["match"]) == want and want and any(n.endswith("/bias") for n in want)
    res = TS.resolve_param_groups(model.entries, [g])
    for n, s, _, t in model.entries:
        if t:
            assert res[n]["weight_decay_scale"] == (0.0 if len(s) <= 1 else 1.0) and res[n]["lr_scale"] == 1.0 and res[n]["trainable"]
    assert "stem_conv/kernel" not in g["match"] and "stem_bn/gamma" in g["match"] and "stem_bn/moving_mean" not in g["match"]


# ---------------------------------------------------------------------------------- the references
def test_the_cases_premises():
    """rectification starts at step 5 and a sync falls on every fifth step: 1, 5 and 6 are the three kinds of step there are"""
    rect = [TS.radam_coeffs(t)["rect"] for t in range(1, 40)]
    assert rect == [False] * 4 + [True] * 35
    assert [t % 5 == 0 for t in PG.ITERATIONS] == [False, True, False] and [TS.radam_coeffs(t)["rect"] for t in PG.ITERATIONS] == [False, True, True]
    A = np.diff(PG.table("A"))
    assert A.max() > 2 * PG.CHUNK and {1023, 1024, 1025} <= set(A.tolist()) and any(o % 4 for o in PG.table("A"))
    assert np.diff(PG.table("B")).tolist() == [5]
    D = np.diff(PG.table("D"))
    assert len(D) > TS.GRAD_GRID_CAP and D[-1] == PG.CHUNK + 1
    for name in PG.TABLES:
        S = len(PG.table(name)) - 1
        c, s = PG.rows(name, "cycle"), PG.rows(name, "shifted")
        assert all(c[i] != c[i + 1] for i in range(S - 1)) and all(s[i] != s[i + 1] for i in range(S - 1))
        assert not PG.rows(name, "default")["frozen"].any()
    long_seg = int(np.argmax(A))
    for s in (0, len(A) - 1, long_seg):
        assert PG.rows("A", "ends")[s]["frozen"] == 1 and (PG.rows("A", "cycle")[s]["frozen"] == 0 or PG.rows("A", "shifted")[s]["frozen"] == 0), s
    assert PG.rows("A", "shifted")[0]["frozen"] == 1 and PG.rows("A", "cycle")[3]["frozen"] == 1 and PG.rows("A", "shifted")[3]["frozen"] == 0
    assert len(PG.CASES) >= 36 and {v for _, _, v in PG.CASES} == set(PG.VARIANTS)


@pytest.mark.parametrize("iteration", PG.ITERATIONS)
@pytest.mark.parametrize("name", ["A", "C"])
def test_reference_with_default_rows_is_the_clipped_step(name, iteration):
    c = PG.vectors(name, "default", "plain")
    seg, rows = PG.table(name), PG.rows(name, "default")
    for coef, wd in ((1.0, PG.WD), (0.75, 0.0)):
        a = dict(m=c["m"].copy(), v=c["v"].copy(), slow=c["slow"].copy(), step=iteration - 1, skipped=0)
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
        ta = TS.clipped_step_reference(c["theta"].copy(), c["grad"], a, PG.LR, coef=coef, weight_decay=wd)
        tb = TS.param_groups_reference(c["theta"].copy(), c["grad"], b, seg, rows, PG.LR, coef=coef, weight_decay=wd)
        assert ta.tobytes() == tb.tobytes() and a["step"] == b["step"] == iteration and b["skipped"] == 0
        for k in ("m", "v", "slow"):
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("iteration", PG.ITERATIONS)
def test_reference_leaves_frozen_segments_and_scales_the_others(iteration):
    c = PG.vectors("A", "cycle", "nan_frozen_grad")
    seg, rows = PG.table("A"), PG.rows("A", "cycle")
    e = PG.expected("A", "cycle", iteration, "nan_frozen_grad")
    for s, r in enumerate(rows):
        lo, hi = int(seg[s]), int(seg[s + 1])
        if r["frozen"]:
            for k in ("theta", "m", "v", "slow"):
                assert e[k][lo:hi].tobytes() == c[k][lo:hi].tobytes(), (s, k)
        else:
            st = dict(m=c["m"].copy(), v=c["v"].copy(), slow=c["slow"].copy(), step=iteration - 1, skipped=0)
            lr, wd = float(np.float32(PG.LR) * r["lr_scale"]), float(np.float32(PG.WD) * r["wd_scale"])
            with np.errstate(invalid="ignore"):
                th = TS.clipped_step_reference(c["theta"].copy(), c["grad"], st, lr, coef=PG.COEF, weight_decay=wd)
            assert e["theta"][lo:hi].tobytes() == th[lo:hi].tobytes() and e["m"][lo:hi].tobytes() == st["m"][lo:hi].tobytes(), s
            assert e["m"][lo:hi].tobytes() != c["m"][lo:hi].tobytes()           # lr_scale = 0 is not frozen: the slots move
    assert all(np.isfinite(e[k]).all() for k in ("theta", "m", "v", "slow")) and e["rec"] == (PG.COEF, 0, 7)
    skipped = PG.expected("A", "cycle", iteration, "nonfinite_skip")
    v = PG.vectors("A", "cycle", "nonfinite_skip")
    assert all(skipped[k].tobytes() == v[k].tobytes() for k in ("theta", "m", "v", "slow")) and skipped["rec"] == (PG.COEF, 2, 8)
    inf = PG.expected("A", "cycle", iteration, "inf_theta")
    assert int(np.isinf(inf["theta"]).sum()) == 1 and not np.isnan(inf["theta"]).any()


def test_mask_reference():
    for name, asg in (("A", "cycle"), ("A", "shifted"), ("D", "cycle")):
        g, seg, rows = PG.mask_gradient(name, asg), PG.table(name), PG.rows(name, asg)
        out = TS.mask_reference(g, seg, rows)
        assert out is not g and out.dtype == np.float32
        for s, r in enumerate(rows):
            lo, hi = int(seg[s]), int(seg[s + 1])
            if r["frozen"]:
                assert not PG.bits(out[lo:hi]).any()                       # +0.0: the word 0
            else:
                assert PG.bits(out[lo:hi]).tobytes() == PG.bits(g[lo:hi]).tobytes()
        frozen = np.concatenate([np.arange(seg[s], seg[s + 1]) for s in range(len(rows)) if rows[s]["frozen"]])
        assert np.isnan(g[frozen]).any() and np.isinf(g[frozen]).any() and (PG.bits(g[frozen]) == 0x80000000).any()
        rest = np.setdiff1d(np.arange(len(g)), frozen)
        assert np.isnan(out[rest]).any() and np.isinf(out[rest]).any() and (PG.bits(out[rest]) == 0x80000000).any()
        assert PG.compare_mask(out, out) == []
    assert TS.mask_reference(PG.mask_gradient("A", "cycle"), PG.table("A"), PG.rows("A", "default")).tobytes() == PG.mask_gradient("A", "cycle").tobytes()


# ---------------------------------------------------------------------------------- the state entry
ENTRIES = [("stem/kernel", (6, 4), 0, True), ("stem/bias", (4,), 24, True), ("bn/moving_mean", (4,), 28, False), ("bn/moving_variance", (4,), 32, False)]


def _state(**kw):
    g = np.random.default_rng(9)
    args = dict(iterations=7, steps=7, step_seed=23774, learning_rate=4e-3, weight_decay=2e-4, apply_weight_decay=True, global_clipnorm=1.5,
                skip_nonfinite=True, accumulate_steps=2, skipped=1)
    args.update(kw)
    return TS.pack_state(ENTRIES, g.standard_normal(36).astype(np.float32), *(g.standard_normal(28).astype(np.float32) for _ in range(3)), **args)


def test_state_entry_round_trips(tmp_path):
    assert TS.PARAM_GROUP_KEYS == ("param_groups",)
    assert set(_state()) == set(_state(param_groups=None)) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS)
    assert "param_groups" not in TS.unpack_state(_state(), ENTRIES)
    groups = [dict(match="*/bias", weight_decay_scale=0.0), dict(match=["stem/*"], lr_scale=0.1, trainable=False)]
    st = _state(param_groups=groups)
    assert set(st) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.PARAM_GROUP_KEYS)
    np.savez(str(tmp_path / "run.npz"), **st)
    with np.load(str(tmp_path / "run.npz"), allow_pickle=False) as z:
        back = TS.unpack_state(z, ENTRIES)
    assert back["param_groups"] == TS.check_param_groups(groups)
    assert TS.resolve_param_groups(ENTRIES, back["param_groups"]) == TS.resolve_param_groups(ENTRIES, groups)
    assert set(_state(param_groups=[], awp_delta=0.2)) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.AWP_KEYS + TS.PARAM_GROUP_KEYS)      # an empty list is set
    with pytest.raises(ValueError, match="matches no trainable entry"):
        _state(param_groups=[dict(match="head/*")])
    with pytest.raises(TS.TrainStateError, match="param_groups"):
        TS.unpack_state(dict(st, param_groups=np.array('[{"match": ["*moving_mean"], "lr_scale": 1.0, "weight_decay_scale": 1.0, "trainable": true}]')), ENTRIES)


# ---------------------------------------------------------------------------------- the Model without a device
def test_changed_by_value_detector(model, monkeypatch):
    from ishara_amd import Optimizer
    import torch
    names = _trainable(model)
    uploads = []

    class _Rows:
        def copy_(self, t):
            uploads.append(t.numpy().view(TS.PARAM_GROUP_DTYPE).copy())

    monkeypatch.setattr(model, "optimizer", Optimizer())
    monkeypatch.setattr(model, "_pg", dict(seg=None, S=len(names), rows=_Rows(), ws=None, frozen=False))
    monkeypatch.setattr(model, "_pg_key", None)
    monkeypatch.setattr(model, "_pg_seen", None)
    assert model._pg_begin_step() is None and uploads == []                            # off: nothing
    model.optimizer.param_groups = [{"match": names[0], "trainable": False}]
    pg = model._pg_begin_step()
    assert pg is model._pg and pg["frozen"] and len(uploads) == 1 and uploads[0][0].tolist() == (1.0, 1.0, 1, 0)
    model.optimizer.param_groups = [dict(match=[names[0]], trainable=False, lr_scale=1.0)]        # another object, the same value
    assert model._pg_begin_step() is pg and len(uploads) == 1
    model.optimizer.param_groups[0]["lr_scale"] = 0.5                                   # changed in place
    model._pg_begin_step()
    assert len(uploads) == 2
    model.optimizer.param_groups = [{"match": "*", "lr_scale": 2.0}]
    assert not model._pg_begin_step()["frozen"] and len(uploads) == 3 and set(uploads[2]["lr_scale"].tolist()) == {2.0}
    assert model.param_groups()[names[3]] == dict(lr_scale=2.0, weight_decay_scale=1.0, trainable=True)
    monkeypatch.setattr(model, "_micro", 1)
    assert model._pg_begin_step() is pg                                                 # unchanged in the middle of a cycle: fine
    model.optimizer.param_groups = [{"match": "*", "lr_scale": 3.0}]
    with pytest.raises(ValueError, match="middle of an accumulation cycle"):
        model._pg_begin_step()
    model.optimizer.param_groups = None
    with pytest.raises(ValueError, match="middle of an accumulation cycle"):
        model._pg_begin_step()
    monkeypatch.setattr(model, "_micro", 0)
    monkeypatch.setattr(model, "_ema_swapped", True)
    with pytest.raises(_lib.IsharaError, match="averaged_weights"):
        model._pg_begin_step()
    monkeypatch.setattr(model, "_ema_swapped", False)
    assert model._pg_begin_step() is None and len(uploads) == 3
    model.optimizer.param_groups = [{"match": "*/kernle"}]
    with pytest.raises(ValueError, match="kernle"):
        model._pg_begin_step()
    assert torch is not None
