"""GPU: the optimizer's parameter groups, from the kernels of csrc/optimizer.hip to Model.

The expected result of a grouped step never comes from the code under test: the plain operator (ishara_optimizer_op_step, which test 1
shows to be the existing step bit for bit) runs once per distinct unfrozen row on copies, with lr' = fp32(lr) * fp32(lr_scale) and
wd' = fp32(wd) * fp32(wd_scale), and the segments are stitched, the frozen ones from the input.  param_groups_parity.compare is on bits
(tests/test_param_groups_mutants.py shows it rejecting the ordinary mistakes).  Every buffer a call writes sits between guard elements.
The model tests use CFGS["tiny"] of test_model_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import param_groups_parity as PG
from ishara_amd import _lib, train_state as TS
from test_model_gpu import CFGS, _build, _oracle_cfg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
F = C.c_float
KEYS = ("theta", "m", "v", "slow")


def _guarded(n, dtype=torch.float32, sentinel=-7.5):
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n], buf


def _intact(buf, n, sentinel=-7.5):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all())


def _rec_tensor(rec):
    """the 16-byte record (norm, coef, nonfinite, skipped) between guards"""
    view, buf = _guarded(4, torch.int32, sentinel=-99)
    raw = np.zeros(4, np.int32)
    raw[:2] = np.array([1.25, rec[0]], np.float32).view(np.int32)
    raw[2:] = rec[1:]
    view.copy_(torch.from_numpy(raw))
    return view, buf


def _read_rec(view):
    raw = view.cpu().numpy()
    assert raw[:1].view(np.float32)[0] == np.float32(1.25)          # norm is not the step's to write
    return float(raw[1:2].view(np.float32)[0]), int(raw[2]), int(raw[3])


class _Slots:
    """theta, grad, m, v, slow of a parity case on the device, each between guards, and the record when the case has one"""

    def __init__(self, c):
        self.n = len(c["theta"])
        self.t, self.bufs = {}, {}
        for k in KEYS + ("grad",):
            self.t[k], self.bufs[k] = _guarded(self.n)
            self.t[k].copy_(torch.from_numpy(c[k].copy()))
            assert self.t[k].data_ptr() % 16 == 0
        self.rec, self.rec_buf = _rec_tensor(c["rec"]) if c["rec"] else (None, None)
        self.skip = 1 if c["skip"] else 0

    def head(self, iteration, lr, wd):
        t = self.t
        return (_lib.ptr(t["theta"]), _lib.ptr(t["grad"]), _lib.ptr(t["m"]), _lib.ptr(t["v"]), _lib.ptr(t["slow"]), self.n, iteration, F(lr), F(wd),
                _lib.ptr(self.rec), self.skip)

    def result(self):
        torch.cuda.synchronize()
        out = {k: self.t[k].cpu().numpy() for k in KEYS}
        out["rec"] = _read_rec(self.rec) if self.rec is not None else None
        out["grad"] = self.t["grad"].cpu().numpy()
        return out

    def intact(self):
        return all(_intact(self.bufs[k], self.n) for k in self.bufs) and (self.rec is None or _intact(self.rec_buf, 4, -99))


def _plain(lib, c, iteration, lr, wd):
    s = _Slots(c)
    _lib.check(lib.ishara_optimizer_op_step(*s.head(iteration, lr, wd), _lib.stream()), "ishara_optimizer_op_step")
    out = s.result()
    assert s.intact()
    return out


def _stitched(lib, c, seg, rows, iteration, lr=PG.LR, wd=PG.WD):
    """the expected grouped step from the plain operator: one run per distinct unfrozen row, frozen segments from the input"""
    base = _plain(lib, c, iteration, lr, wd)                          # the record (and the skip) of a step are those of any plain step
    out = {k: c[k].copy() for k in KEYS}
    out["rec"] = base["rec"]
    runs = {}
    for s, r in enumerate(rows):
        if r["frozen"] != 0:
            continue
        lr_s, wd_s = np.float32(lr) * np.float32(r["lr_scale"]), np.float32(wd) * np.float32(r["wd_scale"])
        key = (lr_s.tobytes(), wd_s.tobytes())
        if key not in runs:
            runs[key] = _plain(lib, c, iteration, float(lr_s), float(wd_s))
        lo, hi = int(seg[s]), int(seg[s + 1])
        for k in KEYS:
            out[k][lo:hi] = runs[key][k][lo:hi]
    return out


class _Grouped:
    def __init__(self, lib, c, seg, rows):
        self.lib, self.c, self.S = lib, c, len(rows)
        self.seg = torch.from_numpy(np.array(seg)).to(DEV)
        self.rows, self.rows_buf = _guarded(4 * self.S, torch.int32, sentinel=-99)
        self.set_rows(rows)
        self.ws_bytes = int(lib.ishara_param_groups_workspace_bytes(len(c["theta"]), self.S))
        assert self.ws_bytes > 0
        self.ws, self.ws_buf = _guarded(self.ws_bytes, torch.uint8, sentinel=0xA5)

    def set_rows(self, rows):
        self.rows.copy_(torch.from_numpy(np.ascontiguousarray(rows).view(np.int32).copy()))

    def step(self, iteration, lr=PG.LR, wd=PG.WD):
        s = _Slots(self.c)
        _lib.check(self.lib.ishara_optimizer_op_step_groups(*s.head(iteration, lr, wd), _lib.ptr(self.seg), _lib.ptr(self.rows), self.S, _lib.ptr(self.ws),
                                                            _lib.stream()), "ishara_optimizer_op_step_groups")
        out = s.result()
        assert s.intact() and _intact(self.rows_buf, 4 * self.S, -99) and _intact(self.ws_buf, self.ws_bytes, 0xA5)
        assert out["grad"].tobytes() == self.c["grad"].tobytes()
        return out


# ---------------------------------------------------------------------------------- models
KW = CFGS["tiny"]
LR = 4e-3


@pytest.fixture(scope="module")
def batches():
    from oracle import ishara_oracle as O
    ocfg = _oracle_cfg(KW, 0.0)
    return [O.synthetic_batch(ocfg, KW["B"], seed=s) for s in (2, 3, 4)]


def _model(dtype, dropout=0.0, seed=3, **opt):
    m = _build(KW, dtype, dropout, seed=seed)
    m.optimizer.learning_rate = LR
    for k, v in opt.items():
        setattr(m.optimizer, k, v)
    return m


def _slots(m):
    return [t.clone() for t in (m.params, m.opt_m, m.opt_v, m.opt_slow)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _case_of(m, rec=None, skip=False):
    """the model's slots and gradient as a parity case (host copies)"""
    nt = m.n_train
    return dict(theta=m.params[:nt].cpu().numpy().copy(), grad=m.grads[:nt].cpu().numpy().copy(), m=m.opt_m.cpu().numpy().copy(),
                v=m.opt_v.cpu().numpy().copy(), slow=m.opt_slow.cpu().numpy().copy(), rec=rec, skip=skip)


def _model_result(m):
    nt = m.n_train
    return dict(theta=m.params[:nt].cpu().numpy(), m=m.opt_m.cpu().numpy(), v=m.opt_v.cpu().numpy(), slow=m.opt_slow.cpu().numpy(), rec=None)


# ---------------------------------------------------------------------------------- 1: the plain operator is the existing step
@pytest.mark.parametrize("with_record", [False, True])
def test_the_plain_operator_is_the_existing_step(lib, batches, with_record):
    m = _model("f32", weight_decay=0.01)
    m.optimizer.apply_weight_decay = True
    if with_record:
        m.optimizer.global_clipnorm = 1e-2                            # far under the gradient's norm: coef != 1
    seen = set()
    for it in range(1, 7):
        m.loss_and_gradients(*batches[it % 3], seed=it)
        before = _case_of(m)
        m.apply_gradients()
        torch.cuda.synchronize()
        if it not in PG.ITERATIONS:
            continue
        rec = None
        if with_record:
            gs = m.grad_stats()
            assert gs["coef"] != 1.0 and gs["nonfinite"] == 0
            rec = (gs["coef"], 0, 0)
        got = _plain(lib, dict(before, rec=rec), it, LR, 0.01)
        assert PG.compare(got, dict(_model_result(m), rec=rec)) == [], it
        seen.add(it)
    assert seen == set(PG.ITERATIONS)


# ---------------------------------------------------------------------------------- 2: the grouped operator against the stitched plain operator
@pytest.mark.parametrize("name,assignment,variant", PG.CASES)
def test_the_grouped_operator_equals_the_stitched_plain_operator(lib, name, assignment, variant):
    c, seg, rows = PG.vectors(name, assignment, variant), PG.table(name), PG.rows(name, assignment)
    g = _Grouped(lib, c, seg, rows)
    for it in PG.ITERATIONS:
        want = _stitched(lib, c, seg, rows, it)
        got = g.step(it)
        assert PG.compare(got, want) == [], it
        assert {k: v.tobytes() for k, v in g.step(it).items() if k != "rec"} == {k: v.tobytes() for k, v in got.items() if k != "rec"}      # a second run
        if variant == "nonfinite_skip":
            assert got["rec"] == (np.float32(PG.COEF), 2, 8) and all(got[k].tobytes() == c[k].tobytes() for k in KEYS)
        if variant == "nan_frozen_grad":
            assert all(np.isfinite(got[k]).all() for k in KEYS)
        if variant == "inf_theta":
            assert int(np.isinf(got["theta"]).sum()) == 1 and not np.isnan(got["theta"]).any()


# ---------------------------------------------------------------------------------- 3: the mask
@pytest.mark.parametrize("assignment", ["cycle", "shifted", "ends"])
@pytest.mark.parametrize("name", ["A", "D"])
def test_the_mask(lib, name, assignment):
    g0, seg, rows = PG.mask_gradient(name, assignment), PG.table(name), PG.rows(name, assignment)
    c = dict(theta=g0, rec=None)
    gr = _Grouped(lib, c, seg, rows)
    g, g_buf = _guarded(len(g0))
    g.copy_(torch.from_numpy(g0.copy()))
    for _ in range(2):                                              # masking a masked gradient changes nothing
        _lib.check(lib.ishara_gradient_mask_groups(None, _lib.ptr(g), len(g0), _lib.ptr(gr.seg), _lib.ptr(gr.rows), gr.S, _lib.ptr(gr.ws), _lib.stream()),
                   "ishara_gradient_mask_groups")
        torch.cuda.synchronize()
        assert PG.compare_mask(g.cpu().numpy(), TS.mask_reference(g0, seg, rows)) == []
        assert _intact(g_buf, len(g0)) and _intact(gr.rows_buf, 4 * gr.S, -99) and _intact(gr.ws_buf, gr.ws_bytes, 0xA5)


# ---------------------------------------------------------------------------------- 4: a model with default rows is the model without groups
PATHS = {
    "plain": dict(),
    "clip_skip": dict(global_clipnorm=0.5, skip_nonfinite=True),
    "accumulate": dict(accumulate_steps=2),
    "awp": dict(awp_delta=0.2),
    "ema": dict(use_ema=True, ema_momentum=0.9),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_default_rows_change_no_bit(batches, path):
    a, b = _model("bf16", 0.2, **PATHS[path]), _model("bf16", 0.2, **PATHS[path])
    b.optimizer.param_groups = [{"match": "*"}]
    calls = 6 if path == "accumulate" else 3
    for i in range(calls):
        la, lb = a.train_on_batch(*batches[i % 3]), b.train_on_batch(*batches[i % 3])
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    assert _same(_slots(a), _slots(b)) and a.optimizer.iterations == b.optimizer.iterations == 3
    if path == "ema":
        assert torch.equal(a._ema_avg, b._ema_avg)
    assert torch.equal(a(batches[0][0]), b(batches[0][0]))          # a forward through the bf16 weight shadows
    assert b._pg is not None and not b._pg["frozen"] and a._pg is None


def test_profiler_keys_of_a_grouped_step(batches):
    m = _model("bf16", 0.0, global_clipnorm=0.5)
    prof = m.profile_step(*batches[0])
    assert prof["radam_lookahead"]["launches"] == 1 and "radam_lookahead_groups" not in prof and "grad_mask_groups" not in prof
    m.optimizer.param_groups = [{"match": "*"}]
    prof = m.profile_step(*batches[0])
    assert (prof["radam_lookahead_groups"]["launches"], prof["radam_lookahead_groups"]["bytes"]) == (1, 28.0 * m.n_train)
    assert "radam_lookahead" not in prof and "grad_mask_groups" not in prof                # nothing frozen: the mask never launches
    m.optimizer.param_groups = [{"match": "stem_conv/*", "trainable": False}]
    prof = m.profile_step(*batches[0])
    assert (prof["grad_mask_groups"]["launches"], prof["grad_mask_groups"]["bytes"]) == (1, 4.0 * m.n_train) and prof["radam_lookahead_groups"]["launches"] == 1
    m.optimizer.awp_delta = 0.2
    assert m.profile_step(*batches[0])["grad_mask_groups"]["launches"] == 2              # in front of the perturbation, and of the statistics


# ---------------------------------------------------------------------------------- 5: a model with real groups equals the composition
def _real_groups(m):
    names = [n for n, _, _, t in m.entries if t]
    block = sorted({n.split("/")[0] for n in names if n.startswith("convsqueeze_0_1")})
    assert block
    head = [n for n in names if n.startswith(names[-1].split("/")[0])]
    return [dict(match=[b + "/*" for b in block], trainable=False), dict(match=head, lr_scale=4.0)] + TS.no_decay_groups(m.entries)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_model_with_groups_equals_the_composition(lib, batches, dtype):
    m = _model(dtype, 0.2, weight_decay=0.01)
    m.optimizer.apply_weight_decay = True
    m.optimizer.param_groups = _real_groups(m)
    seg, rows = TS.param_group_rows(m.entries, m.n_train, m.optimizer.param_groups)
    res = m.param_groups()
    assert any(not r["trainable"] for r in res.values()) and any(r["lr_scale"] == 4.0 for r in res.values())
    assert any(r["weight_decay_scale"] == 0.0 and r["trainable"] for r in res.values()) and len({r.tobytes() for r in rows}) >= 4
    start = _case_of(m)
    for it in range(1, 4):
        m.loss_and_gradients(*batches[it % 3], seed=it)
        before = _case_of(m)
        if it == 1:
            g1 = before["grad"]
        want = _stitched(lib, before, seg, rows, it, LR, 0.01)
        m.apply_gradients()
        torch.cuda.synchronize()
        assert PG.compare(_model_result(m), dict(want, rec=None)) == [], it
    after = _model_result(m)
    for s, r in enumerate(rows):
        lo, hi = int(seg[s]), int(seg[s + 1])
        if r["frozen"]:
            assert all(after[k][lo:hi].tobytes() == start[k][lo:hi].tobytes() for k in KEYS), s
        elif g1[lo:hi].any():                                       # the others move (slow only on a sync step, and there is none in three)
            assert all(after[k][lo:hi].tobytes() != start[k][lo:hi].tobytes() for k in ("theta", "m", "v")), s


# ---------------------------------------------------------------------------------- 6: frozen tensors and the statistics
def _rel(a, b):
    return abs(a - b) / abs(b)


def _frozen_span(m, pattern="convsqueeze_0_1_expand_conv/kernel"):
    (e,) = [(o, int(np.prod(s))) for n, s, o, t in m.entries if n == pattern]
    return e[0], e[0] + e[1]


def test_frozen_tensors_leave_the_statistics(batches):
    pattern = "convsqueeze_0_1_expand_conv/kernel"
    m = _model("f32", global_clipnorm=1e30, skip_nonfinite=True, param_groups=[{"match": pattern, "trainable": False}])
    lo, hi = _frozen_span(m)
    seg, rows = TS.param_group_rows(m.entries, m.n_train, m.optimizer.param_groups)
    m.loss_and_gradients(*batches[0], seed=1)
    g = m.grads[:m.n_train].cpu().numpy().copy()
    start = _slots(m)
    m.apply_gradients()
    got = m.grad_stats()
    want = TS.grad_stats_reference(np.delete(g, np.arange(lo, hi)), 1.0, 1e30)
    full = TS.grad_stats_reference(g, 1.0, 1e30)
    print(f"norm {got['norm']!r} without the frozen tensor {want['norm']!r} with it {full['norm']!r}")
    assert _rel(got["norm"], want["norm"]) <= 1e-6 and _rel(full["norm"], want["norm"]) > 1e-5
    assert PG.compare_mask(m.grads[:m.n_train].cpu().numpy(), TS.mask_reference(g, seg, rows)) == []
    # a NaN in the frozen tensor's gradient: not counted, the step applies
    m.loss_and_gradients(*batches[1], seed=2)
    m.grads[lo + 3] = float("nan")
    before = _slots(m)
    m.apply_gradients()
    got = m.grad_stats()
    assert got["nonfinite"] == 0 and got["skipped"] == 0 and np.isfinite(got["norm"])
    after = _slots(m)
    assert not torch.equal(after[0], before[0]) and all(torch.equal(a[lo:hi], s[lo:hi]) for a, s in zip(after, start))
    assert all(bool(torch.isfinite(t).all()) for t in after)
    # the same NaN in an unfrozen tensor skips the step
    m.loss_and_gradients(*batches[2], seed=3)
    m.grads[hi + 3] = float("nan")
    before = _slots(m)
    m.apply_gradients()
    got = m.grad_stats()
    assert got["nonfinite"] == 1 and got["skipped"] == 1 and _same(_slots(m), before)


# ---------------------------------------------------------------------------------- 7: frozen tensors and AWP
def test_frozen_tensors_and_awp(batches):
    pattern = "convsqueeze_0_1_expand_conv/kernel"
    m = _model("f32", awp_delta=0.2, param_groups=[{"match": pattern, "trainable": False}])
    twin = _model("f32")
    lo, hi = _frozen_span(m)
    seg, rows = TS.param_group_rows(m.entries, m.n_train, m.optimizer.param_groups)
    start = _slots(m)
    x, y = batches[0]
    twin.loss_and_gradients(x, y, seed=5)                           # the pass-1 gradient: same weights, same seed, loss scale 1
    g1 = TS.mask_reference(twin.grads[:twin.n_train].cpu().numpy(), seg, rows)
    _, _, want = TS.awp_reference(twin.params[:twin.n_train].cpu().numpy(), g1, seg, 0.2, 1e-4)
    m.train_on_batch(x, y, seed=5)
    got = m.awp_stats()
    print(f"awp grad_norm {got['grad_norm']!r} reference on the masked gradient {want['grad_norm']!r}")
    assert abs(got["grad_norm"] - want["grad_norm"]) <= 1e-6 * abs(want["grad_norm"]) and got["zeroed"] == 0
    after = _slots(m)
    assert all(torch.equal(a[lo:hi], s[lo:hi]) for a, s in zip(after, start)) and not torch.equal(after[0][:m.n_train], start[0][:m.n_train])
    assert m.awp_scales()[pattern] > 0                               # a zero gradient: a finite scale and a step of 0, not a zeroed tensor


# ---------------------------------------------------------------------------------- 8: off is off
def test_off_is_off(batches):
    m = _model("bf16", 0.0, global_clipnorm=0.5, awp_delta=0.2)
    assert m.optimizer.param_groups is None and m.optimizer.group_options() is None
    prof = m.profile_step(*batches[0])
    m.train_on_batch(*batches[1])
    assert m._pg is None and m._pg_key is None
    assert not any("groups" in k for k in prof) and prof["radam_lookahead"]["launches"] == 1
    assert all(r == dict(lr_scale=1.0, weight_decay_scale=1.0, trainable=True) for r in m.param_groups().values())


# ---------------------------------------------------------------------------------- 9: state
def _resumable(seed, groups=True):
    m = _build(KW, "bf16", 0.2, seed=seed)
    o = m.optimizer
    o.learning_rate, o.global_clipnorm, o.weight_decay, o.apply_weight_decay = LR, 2.0, 0.01, True
    o.use_ema, o.ema_momentum = True, 0.9
    if groups:
        o.param_groups = _real_groups(m)
    return m


def test_resume_is_bit_identical(batches, tmp_path):
    a = _resumable(3)
    for i in range(4):
        a.train_on_batch(*batches[i % 3])
    b = _resumable(3)
    for i in range(2):
        b.train_on_batch(*batches[i % 3])
    path = b.save_state(str(tmp_path / "state"))
    with np.load(path) as z:
        assert set(z.files) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.EMA_KEYS + TS.PARAM_GROUP_KEYS)
    c = _resumable(99, groups=False)
    c.load_state(path)
    assert c.optimizer.group_options() == b.optimizer.group_options() and c.param_groups() == a.param_groups()
    for i in range(2, 4):
        c.train_on_batch(*batches[i % 3])
    assert _same(_slots(a), _slots(c)), "the resumed run left the uninterrupted one"
    assert torch.equal(a._ema_avg, c._ema_avg) and a.grad_stats() == c.grad_stats()
    plain = _resumable(3, groups=False)                            # a state without groups has the keys it had, and leaves the option alone
    plain.train_on_batch(*batches[0])
    with np.load(plain.save_state(str(tmp_path / "plain"))) as z:
        assert set(z.files) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.EMA_KEYS)
    c.load_state(str(tmp_path / "plain"))
    assert c.optimizer.group_options() == b.optimizer.group_options()


# ---------------------------------------------------------------------------------- 10: graph capture
def test_graph_capture_replays_and_follows_the_rows(lib):
    """the mask and the grouped operator in one linear chain; rows changed on the device take effect without a new capture"""
    name, it = "A", 5
    c, seg = PG.vectors(name, "cycle", "nonfinite_skip"), PG.table(name)
    c = dict(c, rec=(PG.COEF, 0, 7))                                  # the switch on, not taken
    rows_a, rows_b = PG.rows(name, "cycle"), PG.rows(name, "ends")
    gr = _Grouped(lib, c, seg, rows_a)
    s = _Slots(c)
    init = {k: s.t[k].clone() for k in s.t}

    def load():
        for k in s.t:
            s.t[k].copy_(init[k])

    def chain():
        _lib.check(lib.ishara_gradient_mask_groups(None, _lib.ptr(s.t["grad"]), s.n, _lib.ptr(gr.seg), _lib.ptr(gr.rows), gr.S, _lib.ptr(gr.ws), _lib.stream()),
                   "ishara_gradient_mask_groups")
        _lib.check(lib.ishara_optimizer_op_step_groups(*s.head(it, PG.LR, PG.WD), _lib.ptr(gr.seg), _lib.ptr(gr.rows), gr.S, _lib.ptr(gr.ws), _lib.stream()),
                   "ishara_optimizer_op_step_groups")

    eager = {}
    for key, rows in (("b", rows_b), ("a", rows_a)):                  # eager runs (they also load the kernels before the capture)
        gr.set_rows(rows)
        load()
        chain()
        eager[key] = s.result()
        assert PG.compare(eager[key], _stitched(lib, c, seg, rows, it)) == []
        assert PG.compare_mask(eager[key]["grad"], TS.mask_reference(c["grad"], seg, rows)) == []
    load()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for key, rows in (("a", rows_a), ("b", rows_b)):
        load()
        gr.rows.copy_(torch.from_numpy(np.ascontiguousarray(rows).view(np.int32).copy()).to(DEV))      # on the device, no new capture
        gr.ws.zero_()
        graph.replay()
        got = s.result()
        assert PG.compare(got, eager[key]) == [] and got["grad"].tobytes() == eager[key]["grad"].tobytes(), key
        assert s.intact()
    assert PG.compare(eager["a"], eager["b"]) != []
