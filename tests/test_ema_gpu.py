"""GPU: the exponential moving average of the weights, from the two streaming kernels of csrc/weight_avg.hip (against
train_state.ema_reference bit for bit on the vectors and scenarios of ema_parity.py, with guard elements on both sides of every buffer)
through the refusals of the two entry points to Model: train_on_batch on both step paths, skipped steps, accumulation cycles,
averaged_weights(), the overwrite, save_state / load_state, graph capture, fit, evaluate, save_weights and CallbackEval.  The model tests use
CFGS["tiny"] of test_model_gpu.py.

Everything is compared bit for bit: the update is three fp32 roundings the numpy restatement reproduces exactly (tests/test_ema_mutants.py
shows the comparison rejecting an FMA, the two-product form and the counter mistakes on these vectors), and a swap moves words."""
import ctypes as C

import numpy as np
import pytest
import torch

import ema_parity as EP
from ishara_amd import _lib, train_state as TS
from test_model_gpu import CFGS, _build, _oracle_cfg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
F = C.c_float
BIG = EP.SIZES[-1]


def _guarded(n, dtype=torch.float32, sentinel=-7.5):
    """a [n] view at 16-byte alignment with GUARD sentinel elements on each side -> (view, whole buffer)"""
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n], buf


def _intact(buf, n, sentinel=-7.5):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all())


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class _Buffers:
    """avg, theta, the ema record and a grad-stats record, each between guards"""

    def __init__(self, n):
        self.n = n
        self.avg, self.avg_buf = _guarded(n)
        self.theta, self.theta_buf = _guarded(n)
        self.rec, self.rec_buf = _guarded(2, torch.int64, sentinel=-99)
        self.st, self.st_buf = _guarded(4, torch.int32, sentinel=-99)
        self.rec.zero_()
        self.st.zero_()

    def intact(self):
        return (_intact(self.avg_buf, self.n) and _intact(self.theta_buf, self.n) and _intact(self.rec_buf, 2, -99) and _intact(self.st_buf, 4, -99))

    def state(self):
        raw = self.rec.cpu().numpy()
        return dict(updates=int(raw[0]), alpha=raw[1:].view(np.float32)[0], overwrote=int(raw[1:].view(np.int32)[1]))

    def snap(self):
        return EP.snap(self.avg.cpu().numpy(), self.theta.cpu().numpy(), self.state())


def _launch(lib, b, sc, skip, st=True):
    _lib.check(lib.ishara_weight_average(None, _lib.ptr(b.avg), _lib.ptr(b.theta), b.n, F(EP.MOMENTUM), 1 if sc["warmup"] else 0, sc["every"],
                                         _lib.ptr(b.rec), _lib.ptr(b.st) if st else None, skip, _lib.stream()), "ishara_weight_average")


def _play(lib, n, sc):
    """the scenario on the device -> (snapshots after every launch, the buffers)"""
    avg0, thetas = EP.vectors(n)
    b = _Buffers(n)
    b.avg.copy_(torch.from_numpy(avg0.copy()))
    uses_st = any(nf or sk for nf, sk in sc["launches"])       # a scenario without a skipped step passes st = NULL
    out = []
    for k, (nonfinite, skip) in enumerate(sc["launches"]):
        b.theta.copy_(torch.from_numpy(thetas[k % 3].copy()))
        b.st[2] = nonfinite
        _launch(lib, b, sc, skip, st=uses_st)
        out.append(b.snap())
    return out, b


# ---------------------------------------------------------------------------------- 1, 2, 3: the update against the reference
@pytest.mark.parametrize("n", EP.SIZES)
@pytest.mark.parametrize("name", ["plain", "warmup", "overwrite2", "skipped", "skipped_overwrite"])
def test_weight_average_equals_the_reference(lib, name, n):
    sc = EP.SCENARIOS[name]
    got, b = _play(lib, n, sc)
    want = EP.reference(n, name)
    assert EP.same(got, want), EP.first_difference(got, want)
    assert b.intact()
    if sc["every"] == 0:                                       # theta is read only: what was written into it is what it holds
        thetas = EP.vectors(n)[1]
        assert all(s["theta"] == thetas[k % 3].tobytes() for k, s in enumerate(got))


def test_overwrite_every_second_update(lib):
    for n in (5, 1025, BIG):
        got, _ = _play(lib, n, EP.SCENARIOS["overwrite2"])
        thetas = EP.vectors(n)[1]
        assert [s["overwrote"] for s in got] == [0, 1, 0, 1] and [s["updates"] for s in got] == [1, 2, 3, 4]
        for k, s in enumerate(got):
            assert (s["theta"] == s["avg"]) == (k in (1, 3)), k
            if k in (0, 2):
                assert s["theta"] == thetas[k % 3].tobytes()


def test_skipped_step_leaves_the_average_alone(lib):
    for n in (5, 1025, BIG):
        got, _ = _play(lib, n, EP.SCENARIOS["skipped"])
        first, skipped, unguarded = got
        assert skipped["avg"] == first["avg"] and skipped["updates"] == first["updates"] == 1 and skipped["alpha"] == first["alpha"]
        assert skipped["overwrote"] == 0
        assert unguarded["updates"] == 2 and unguarded["avg"] != first["avg"]      # skip_nonfinite = 0: the same record does not stop it
        got, _ = _play(lib, n, EP.SCENARIOS["skipped_overwrite"])
        assert [s["updates"] for s in got] == [1, 1, 2, 3] and [s["overwrote"] for s in got] == [0, 0, 1, 0]
        assert got[1]["theta"] == EP.vectors(n)[1][1].tobytes()                    # the skipped launch did not overwrite theta either


# ---------------------------------------------------------------------------------- 4: the counter
def test_back_to_back_launches_count_in_order(lib):
    """50 launches on one stream at the largest size (2048 workgroups, two grid-stride rounds) with warm-up on and no host synchronise
    between them: every workgroup of launch k must have read updates = k - 1.  A counter advanced inside the update kernel would hand
    late workgroups another alpha."""
    sc = EP.SCENARIOS["ordering"]
    avg0, thetas = EP.vectors(BIG)
    b = _Buffers(BIG)
    b.avg.copy_(torch.from_numpy(avg0.copy()))
    b.theta.copy_(torch.from_numpy(thetas[0].copy()))
    torch.cuda.synchronize()
    for _ in sc["launches"]:
        _launch(lib, b, sc, 0, st=False)
    torch.cuda.synchronize()
    got, want = b.snap(), EP.reference(BIG, "ordering")[-1]
    assert got["updates"] == 50
    assert EP.same([got], [want]), EP.first_difference([got], [want])
    assert b.intact()


# ---------------------------------------------------------------------------------- 5: the swap
@pytest.mark.parametrize("n", EP.SIZES)
def test_weight_swap_exchanges_every_bit(lib, n):
    a0, b0 = EP.bit_patterns(n)
    a, abuf = _guarded(n, torch.int32, sentinel=-99)
    b, bbuf = _guarded(n, torch.int32, sentinel=-99)
    a.copy_(torch.from_numpy(a0.view(np.int32).copy()))
    b.copy_(torch.from_numpy(b0.view(np.int32).copy()))
    _lib.check(lib.ishara_weight_swap(None, _lib.ptr(a), _lib.ptr(b), n, _lib.stream()), "ishara_weight_swap")
    assert EP.swap_same(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32), a0, b0)
    assert _intact(abuf, n, -99) and _intact(bbuf, n, -99)
    _lib.check(lib.ishara_weight_swap(None, _lib.ptr(a), _lib.ptr(b), n, _lib.stream()), "ishara_weight_swap")
    assert a.cpu().numpy().view(np.uint32).tobytes() == a0.tobytes() and b.cpu().numpy().view(np.uint32).tobytes() == b0.tobytes()
    assert _intact(abuf, n, -99) and _intact(bbuf, n, -99)


# ---------------------------------------------------------------------------------- 6: refusals
def test_refusals_leave_the_buffers_untouched(lib):
    n = 1025
    avg0, thetas = EP.vectors(n)
    b = _Buffers(n)
    b.avg.copy_(torch.from_numpy(avg0.copy()))
    b.theta.copy_(torch.from_numpy(thetas[0].copy()))
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    name = "ishara_weight_average"

    def avg_call(avg=P(b.avg), theta=P(b.theta), n=n, momentum=0.9, every=0, rec=P(b.rec), st=None, skip=0):
        return lib.ishara_weight_average(None, avg, theta, n, F(momentum), 1, every, rec, st, skip, _lib.stream())

    def swap_call(x=P(b.avg), y=P(b.theta), n=n):
        return lib.ishara_weight_swap(None, x, y, n, _lib.stream())
    calls = [(name, c) for c in (
        lambda: avg_call(n=0), lambda: avg_call(n=-3), lambda: avg_call(n=2 ** 31),
        lambda: avg_call(avg=None), lambda: avg_call(theta=None), lambda: avg_call(rec=None),
        lambda: avg_call(avg=P(b.avg, 4)), lambda: avg_call(theta=P(b.theta, 8)), lambda: avg_call(rec=P(b.rec, 4)),
        lambda: avg_call(theta=P(b.avg)), lambda: avg_call(theta=P(b.avg, 16), n=n - 4), lambda: avg_call(avg=P(b.theta, 16), n=n - 4),
        lambda: avg_call(momentum=1.0), lambda: avg_call(momentum=-0.5), lambda: avg_call(momentum=float("nan")),
        lambda: avg_call(every=-1), lambda: avg_call(skip=1))]
    calls += [("ishara_weight_swap", c) for c in (
        lambda: swap_call(n=0), lambda: swap_call(n=2 ** 31), lambda: swap_call(x=None), lambda: swap_call(y=None),
        lambda: swap_call(x=P(b.avg, 4)), lambda: swap_call(y=P(b.theta, 12)), lambda: swap_call(y=P(b.avg)), lambda: swap_call(y=P(b.avg, 16), n=n - 4))]
    for i, (who, call) in enumerate(calls):
        rc = call()
        msg = (lib.ishara_last_error() or b"").decode()
        assert rc != 0 and msg.startswith(who + ":"), (i, rc, msg)
    torch.cuda.synchronize()
    assert b.avg.cpu().numpy().tobytes() == avg0.tobytes() and b.theta.cpu().numpy().tobytes() == thetas[0].tobytes()
    assert b.state() == dict(updates=0, alpha=0.0, overwrote=0) and b.intact()


# ---------------------------------------------------------------------------------- models
KW = CFGS["tiny"]
LR = 4e-3


@pytest.fixture(scope="module")
def batches():
    from oracle import ishara_oracle as O
    ocfg = _oracle_cfg(KW, 0.0)
    return [O.synthetic_batch(ocfg, KW["B"], seed=s) for s in (2, 3, 4)]


def _ema_model(dtype, dropout=0.0, seed=3, **ema):
    m = _build(KW, dtype, dropout, seed=seed)
    m.optimizer.learning_rate = LR
    m.optimizer.use_ema = True
    for k, v in ema.items():
        setattr(m.optimizer, k, v)
    return m


def _prefix(m):
    return m.params[:m.n_train].cpu().numpy().copy()


def _flat(m, weights):
    """a get_weights-style dict laid out as the flat parameter buffer"""
    flat = np.zeros(m.n_total, np.float32)
    for n, s, o, _ in m.entries:
        flat[o:o + int(np.prod(s))] = np.asarray(weights[n], np.float32).reshape(-1)
    return flat


def _slots(m):
    return [t.clone() for t in (m.params, m.opt_m, m.opt_v, m.opt_slow)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_model_average_follows_the_reference(batches):
    """7: six steps of the default step path (ishara_optimizer_step), momentum 0.9, warm-up on"""
    m = _ema_model("f32", ema_momentum=0.9, ema_warmup=True)
    nt = m.n_train
    avg, st = _prefix(m), TS.ema_state_init()                  # Keras: the average starts at the variable
    for step in range(6):
        m.train_on_batch(*batches[step % 3], seed=step)
        avg, _ = TS.ema_reference(avg, _prefix(m), st, 0.9, warmup=True)
        flat = _flat(m, m.ema_weights())
        assert flat[:nt].tobytes() == avg.tobytes(), f"step {step + 1}"
        assert flat[nt:].tobytes() == m.params[nt:].cpu().numpy().tobytes()          # the BatchNorm statistics are the live ones
        got = m.ema_state()
        assert got["updates"] == step + 1 and np.float32(got["alpha"]) == st["alpha"] and got["overwrote"] == 0
    assert m._gstats is None                                   # the default path: no grad-stats record was needed
    assert not np.array_equal(avg, _prefix(m))


def test_model_skipped_step(batches):
    """8: the record path; a NaN in the gradient skips the step and the average with it"""
    m = _ema_model("f32", ema_momentum=0.9, ema_warmup=True)
    m.optimizer.skip_nonfinite = True
    x, y = batches[0]
    avg, st = _prefix(m), TS.ema_state_init()
    m.train_on_batch(x, y, seed=0)
    avg, _ = TS.ema_reference(avg, _prefix(m), st, 0.9, warmup=True)
    assert m._ema_avg.cpu().numpy().tobytes() == avg.tobytes() and m.ema_state()["updates"] == 1
    m.loss_and_gradients(x, y, seed=1)
    m.grads[m.n_train // 2] = float("nan")                     # a memory write from torch; nothing faults
    theta = _prefix(m)
    m.apply_gradients()
    assert m.grad_stats()["skipped"] == 1 and _prefix(m).tobytes() == theta.tobytes()
    got = m.ema_state()
    assert m._ema_avg.cpu().numpy().tobytes() == avg.tobytes() and got["updates"] == 1 and got["overwrote"] == 0
    assert np.float32(got["alpha"]) == st["alpha"]
    m.train_on_batch(x, y, seed=2)
    avg, _ = TS.ema_reference(avg, _prefix(m), st, 0.9, warmup=True)
    assert m._ema_avg.cpu().numpy().tobytes() == avg.tobytes() and m.ema_state()["updates"] == 2


def test_model_accumulation_updates_once_per_cycle(batches):
    """9"""
    m = _ema_model("f32", ema_momentum=0.9)
    m.optimizer.accumulate_steps = 2
    avg, st = _prefix(m), TS.ema_state_init()
    for j in range(4):
        m.train_on_batch(*batches[j % 3], seed=j)
        if j == 0:
            assert m._ema_avg is None                          # no step has been applied yet
        if j % 2 == 1:
            avg, _ = TS.ema_reference(avg, _prefix(m), st, 0.9)
        if j >= 1:
            assert m.ema_state()["updates"] == (j + 1) // 2, j
            assert m._ema_avg.cpu().numpy().tobytes() == avg.tobytes(), j
    assert m.optimizer.iterations == 2


def test_averaged_weights_context(batches):
    """10: bf16, so the forward reads the 16-bit weight shadows: equal outputs prove they were refreshed"""
    m = _ema_model("bf16", ema_momentum=0.9)
    x, y = batches[0]
    nt = m.n_train
    fresh = _build(KW, "bf16", 0.0, seed=99)
    with pytest.raises(_lib.IsharaError, match="no moving average"):
        with fresh.averaged_weights():
            pass
    for step in range(3):
        m.train_on_batch(*batches[step], seed=step)
    before, out_before = m.params.clone(), m(x).clone()
    avg = m._ema_avg.clone()
    assert not torch.equal(before[:nt], avg)
    fresh.set_weights(m.ema_weights())
    want = fresh(x).clone()
    assert not torch.equal(want, out_before)
    with m.averaged_weights() as inside:
        assert inside is m
        assert torch.equal(m.params[:nt], avg) and torch.equal(m.params[nt:], before[nt:])
        assert torch.equal(m._ema_avg, before[:nt])
        assert torch.equal(m(x), want), "the forward inside the context is not the averaged model's"
        assert _flat(m, m.ema_weights()).tobytes() == m.params.cpu().numpy().tobytes()
        with pytest.raises(_lib.IsharaError, match="inside averaged_weights"):
            m.train_on_batch(x, y)
        with pytest.raises(_lib.IsharaError, match="inside averaged_weights"):
            m.apply_gradients()
        with pytest.raises(_lib.IsharaError, match="already inside"):
            with m.averaged_weights():
                pass
        with pytest.raises(_lib.IsharaError, match="inside averaged_weights"):
            m.finalize_ema()
        assert torch.equal(m.params[:nt], avg)                 # the refusals changed nothing
    assert torch.equal(m.params, before) and torch.equal(m._ema_avg, avg)
    assert torch.equal(m(x), out_before)
    with pytest.raises(RuntimeError, match="boom"):
        with m.averaged_weights():
            raise RuntimeError("boom")
    assert torch.equal(m.params, before) and torch.equal(m._ema_avg, avg) and torch.equal(m(x), out_before)
    m.train_on_batch(x, y, seed=9)                             # and training goes on
    assert m.ema_state()["updates"] == 4


def test_overwrite_refreshes_the_weight_shadows(batches):
    """11"""
    m = _ema_model("bf16", ema_momentum=0.9, ema_overwrite_frequency=2)
    x, y = batches[0]
    nt = m.n_train
    m.train_on_batch(x, y, seed=0)
    assert m.ema_state()["overwrote"] == 0 and not torch.equal(m.params[:nt], m._ema_avg)
    m.train_on_batch(*batches[1], seed=1)
    assert m.ema_state() == dict(updates=2, alpha=float(TS.ema_alpha(1, 0.9)), overwrote=1)
    assert torch.equal(m.params[:nt], m._ema_avg)
    fresh = _build(KW, "bf16", 0.0, seed=99)
    fresh.set_weights(m.get_weights())
    assert torch.equal(m(x), fresh(x)), "the forward after an overwrite does not use the overwritten weights"


def _resumable(seed, use_ema=True):
    m = _build(KW, "bf16", 0.2, seed=seed)
    m.optimizer.learning_rate = LR
    m.optimizer.global_clipnorm = 2.0
    if use_ema:
        o = m.optimizer
        o.use_ema, o.ema_momentum, o.ema_warmup, o.ema_overwrite_frequency = True, 0.95, True, 4
    return m


def test_resume_is_bit_identical_with_the_average(batches, tmp_path):
    """12: A trains 6 steps; B trains 3 and saves; C, built from another seed and without the ema settings, loads and trains 3 more.  The
    overwrite at update 4 and the warm-up's alpha only agree if the counter came back."""
    a = _resumable(3)
    for i in range(6):
        a.train_on_batch(*batches[i % 3])
    b = _resumable(3)
    for i in range(3):
        b.train_on_batch(*batches[i % 3])
    path = b.save_state(str(tmp_path / "state"))
    with np.load(path) as z:
        assert set(z.files) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.EMA_KEYS)
    c = _resumable(99, use_ema=False)
    c.load_state(path)
    assert c.optimizer.ema_options() == b.optimizer.ema_options() == (True, 0.95, 4, True)
    assert torch.equal(c._ema_avg, b._ema_avg) and c.ema_state()["updates"] == 3
    for i in range(3, 6):
        c.train_on_batch(*batches[i % 3])
    assert _same(_slots(a), _slots(c)), "the resumed run left the uninterrupted one"
    assert torch.equal(a._ema_avg, c._ema_avg)
    assert a.ema_state() == c.ema_state() and a.ema_state()["updates"] == 6


def test_state_without_the_average_starts_a_fresh_one(batches, tmp_path):
    """13"""
    b = _resumable(3, use_ema=False)
    for i in range(2):
        b.train_on_batch(*batches[i])
    path = b.save_state(str(tmp_path / "plain"))
    c = _resumable(99)
    c.train_on_batch(*batches[0])                              # an average of its own, which the load replaces
    assert c.ema_state()["updates"] == 1
    c.load_state(path)
    assert torch.equal(c.params, b.params) and torch.equal(c._ema_avg, c.params[:c.n_train])
    assert c.ema_state() == dict(updates=0, alpha=0.0, overwrote=0)
    assert c.optimizer.ema_options() == (True, 0.95, 4, True)  # a file without the keys leaves the settings alone


def test_graph_capture_replays_the_eager_cycle(lib, batches):
    """14: grad_stats -> optimizer_step_ex -> weight_average on one stream (no side stream, so no parallel branches)"""
    m = _ema_model("f32", ema_momentum=0.9, ema_warmup=True)
    x, y = batches[0]
    m.loss_and_gradients(x, y, seed=1)
    src = m.grads[:m.n_train]
    before = _slots(m)

    def cycle():
        m._launch_grad_stats(src, 1.0, 0.01)
        m._apply_gradients_ex(src, True)
    cycle()                                                    # eager (also creates the average and loads the kernels before the capture)
    torch.cuda.synchronize()
    eager, eager_avg, eager_rec, eager_gs = _slots(m), m._ema_avg.clone(), m._ema_rec.clone(), m._gstats.clone()
    assert not torch.equal(eager[0], before[0]) and not torch.equal(eager_avg, before[0][:m.n_train])
    assert m.ema_state()["updates"] == 1

    def rewind():
        for t, s in zip((m.params, m.opt_m, m.opt_v, m.opt_slow), before):
            t.copy_(s)
        m._ema_avg.copy_(before[0][:m.n_train])
        m._ema_rec.zero_()
        m._gstats.zero_()
        _lib.check(lib.ishara_optimizer_set_iterations(m._h, 0))
    rewind()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cycle()
    rewind()                                                   # the capture ran nothing, but consumed an iteration number on the host
    graph.replay()
    torch.cuda.synchronize()
    assert _same(eager, _slots(m)) and torch.equal(eager_gs, m._gstats)
    assert torch.equal(eager_avg, m._ema_avg) and torch.equal(eager_rec, m._ema_rec)


def test_fit_evaluate_save_and_callback(batches, tmp_path):
    """15"""
    from ishara_amd.evaluation import CallbackEval, make_num_to_char
    m = _ema_model("bf16", ema_momentum=0.9)
    nt = m.n_train
    for step in range(3):
        m.train_on_batch(*batches[step], seed=step)
    ds = batches[:2]
    live, averaged = m.evaluate(ds), m.evaluate(ds, averaged=True)
    assert live != averaged
    from ishara_amd import keras_h5
    for ext in ("npz", "h5") if keras_h5.available() else ("npz",):      # every format save_weights writes in this environment
        path = str(tmp_path / f"avg.{ext}")
        m.save_weights(path, averaged=True)
        other = _build(KW, "bf16", 0.0, seed=99)
        other.load_weights(path)
        assert torch.equal(other.params[:nt], m._ema_avg) and torch.equal(other.params[nt:], m.params[nt:])
        assert other.evaluate(ds) == averaged, ext
    num_to_char = make_num_to_char({chr(ord("a") + i % 26) + str(i // 26): i for i in range(59)})
    lines = []
    cb = CallbackEval([batches[0]], num_to_char, n_show=1, weights_path=str(tmp_path / "cb.npz"), printer=lines.append, averaged=True)
    cb.set_model(m)
    before = m.params.clone()
    cb.on_epoch_end(0, {})
    assert torch.equal(m.params, before) and not m._ema_swapped and lines
    with np.load(str(tmp_path / "cb.npz")) as z:               # the callback's weights file holds the averaged model
        assert _flat(m, {k: z[k] for k in z.files})[:nt].tobytes() == m._ema_avg.cpu().numpy().tobytes()
    logits = m(batches[0][0]).clone()
    with m.averaged_weights():
        want = ["".join(num_to_char.get(int(i), "") for i in idx) for idx in m.decode_batch(m(batches[0][0]))]
    got = [l[len("Prediction: "):].rsplit(", len: ", 1)[0] for l in lines if l.startswith("Prediction: ")]
    assert got == want[:1] and torch.equal(m(batches[0][0]), logits)
    ended = []

    class AtEnd:
        def set_model(self, model): self.model = model
        def on_train_begin(self, logs=None): pass
        def on_epoch_begin(self, epoch, logs=None): pass
        def on_epoch_end(self, epoch, logs=None): ended.append(("epoch", torch.equal(self.model.params[:nt], self.model._ema_avg)))
        def on_train_end(self, logs=None): ended.append(("end", torch.equal(self.model.params[:nt], self.model._ema_avg)))
    h = m.fit(batches, epochs=2, verbose=0, callbacks=[AtEnd()])
    assert h.history["ema_updates"] == [6, 9]
    assert ended == [("epoch", False), ("epoch", False), ("end", True)]      # finalised after the last epoch, before on_train_end
    assert torch.equal(m.params[:nt], m._ema_avg)
    fresh = _build(KW, "bf16", 0.0, seed=99)
    fresh.set_weights(m.get_weights())
    assert torch.equal(m(batches[0][0]), fresh(batches[0][0]))                 # the shadows hold the finalised weights


def test_defaults_touch_nothing(batches, tmp_path):
    """16: use_ema off: neither step path creates a buffer or a record, the state file has exactly the keys it had"""
    m = _build(KW, "bf16", 0.0)
    m.train_on_batch(*batches[0])                              # ishara_optimizer_step
    m.optimizer.global_clipnorm = 1.0
    m.train_on_batch(*batches[1])                              # ishara_optimizer_step_ex
    h = m.fit(batches, epochs=1, verbose=0)
    assert m._ema_avg is None and m._ema_rec is None and "ema_updates" not in h.history
    with np.load(m.save_state(str(tmp_path / "state"))) as z:
        assert set(z.files) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS)
    prof = m.profile_step(*batches[0])
    assert "weight_average" not in prof and "weight_swap" not in prof
    m.optimizer.use_ema = True
    prof = m.profile_step(*batches[0])
    assert prof["weight_average"]["launches"] == 1 and prof["weight_average"]["bytes"] == 12.0 * m.n_train
    with pytest.raises(_lib.IsharaError, match="no moving average"):
        _build(KW, "bf16", 0.0).ema_weights()
