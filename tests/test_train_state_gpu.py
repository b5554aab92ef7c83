"""GPU: global-norm gradient clipping, the non-finite guard, microbatch accumulation and the resumable training state, from the two streaming
kernels of csrc/grad_ops.hip (against fp64 numpy / fp32 torch at the launcher's edges, with guard elements) through
ishara_optimizer_step_ex (legacy identity, clipped steps against the restated algorithm, skipped steps) to Model.train_on_batch, fit,
save_state / load_state and graph capture.  The model tests use CFGS["tiny"] of test_model_gpu.py.

Bounds: the norm at relative 1e-6 (an fp64 sum of <= 1e7 terms contributes < 1e-9, the rest is the fp32 store); coef at 1e-6 (three fp32
roundings); parameters after a step within 2e-6 * (1 + max|theta|), the bound test_optimizer_parity uses for this update; everything said
to be identical is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from ishara_amd import _lib, train_state as TS
from test_model_gpu import CFGS, _build, _oracle_cfg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPAN, CAP = TS.GRAD_WG_SPAN, TS.GRAD_GRID_CAP
SIZES = sorted({1, 3, 4, 255, 256, 257, 1023, 1025, SPAN - 1, SPAN + 1, CAP * SPAN + 5})
GUARD = 64
F = C.c_float


def _guarded(n, dtype=torch.float32, sentinel=-7.5):
    """a [n] view at 16-byte alignment with GUARD sentinel elements on each side -> (view, whole buffer)"""
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n], buf


def _intact(buf, n, sentinel=-7.5):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all())


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def ws():
    """one workspace for every grad_stats call of this module: 0xFF bytes before its first use, never cleared between calls"""
    return torch.full((TS.grad_stats_workspace_bytes(max(SIZES)),), 0xFF, dtype=torch.uint8, device=DEV)


@pytest.fixture(scope="module")
def vectors():
    """N(0,1) vectors per size (three each: the accumulate test adds them), generated once"""
    g = torch.Generator().manual_seed(1234)
    return {n: [torch.randn(n, generator=g, dtype=torch.float32) for _ in range(3)] for n in SIZES}


def _stats(lib, g, scale, clip, ws, rec=None):
    rec = torch.zeros(4, dtype=torch.int32, device=DEV) if rec is None else rec
    _lib.check(lib.ishara_gradient_stats(None, _lib.ptr(g), g.numel(), F(scale), F(clip), _lib.ptr(rec), _lib.ptr(ws), _lib.stream()), "ishara_gradient_stats")
    raw = rec.cpu().numpy()
    f = raw.view(np.float32)
    return dict(norm=float(f[0]), coef=float(f[1]), nonfinite=int(raw[2]), skipped=int(raw[3]), raw=raw.tobytes())


def _rel(a, b):
    return abs(a - b) / abs(b)


# ---------------------------------------------------------------------------------- 1, 3: grad_stats
@pytest.mark.parametrize("n", SIZES)
def test_grad_stats_against_fp64(lib, ws, vectors, n):
    host = vectors[n][0]
    g, gbuf = _guarded(n)
    g.copy_(host)
    ref = float(np.sqrt(np.sum(host.numpy().astype(np.float64) ** 2)))
    a = _stats(lib, g, 1.0, 0.0, ws)
    print(f"n={n}: norm {a['norm']!r} ref {ref!r} rel {_rel(a['norm'], ref):.2e}")
    assert _rel(a["norm"], ref) <= 1e-6
    assert a["coef"] == 1.0 and a["nonfinite"] == 0 and a["skipped"] == 0
    assert _stats(lib, g, 1.0, 0.0, ws)["raw"] == a["raw"], "two runs differ"
    hi = _stats(lib, g, 1.0, 2.0 * ref, ws)                 # norm under the clip: exactly 1
    assert hi["coef"] == 1.0 and hi["norm"] == a["norm"]
    lo = _stats(lib, g, 1.0, 0.5 * ref, ws)
    assert _rel(lo["coef"], 0.5 * ref / (ref + 1e-6)) <= 1e-6 and lo["coef"] < 1.0
    half = _stats(lib, g, 0.5, 0.25 * ref, ws)              # grad_scale 1/2: norm of the mean gradient, coef = scale * clip / norm
    assert _rel(half["norm"], 0.5 * ref) <= 1e-6 and _rel(half["coef"], 0.5 * 0.25 * ref / (0.5 * ref + 1e-6)) <= 1e-6
    want = TS.grad_stats_reference(host.numpy(), 0.5, 0.25 * ref)
    assert _rel(half["norm"], want["norm"]) <= 1e-6 and _rel(half["coef"], want["coef"]) <= 1e-6
    assert _intact(gbuf, n) and torch.equal(g.cpu(), host)


def test_grad_stats_overflow_needs_fp64(lib, ws):
    g = torch.full((1000,), 3e19, dtype=torch.float32, device=DEV)
    want = float(np.float32(3e19)) * np.sqrt(1000.0)
    a = _stats(lib, g, 1.0, 1.0, ws)
    print(f"overflow: norm {a['norm']!r} want {want!r}")
    assert np.isfinite(a["norm"]) and _rel(a["norm"], want) <= 1e-6
    assert a["nonfinite"] == 0 and _rel(a["coef"], 1.0 / want) <= 1e-6


def test_grad_stats_counts_nonfinite(lib, ws, vectors):
    g = vectors[1025][0].to(DEV)
    g[0], g[1024], g[300], g[777] = float("nan"), float("inf"), float("inf"), float("-inf")
    a = _stats(lib, g, 1.0, 1.0, ws)
    assert a["nonfinite"] == 4 and np.isnan(a["norm"])
    g[0] = 0.0
    b = _stats(lib, g, 1.0, 1.0, ws)
    assert b["nonfinite"] == 3 and np.isinf(b["norm"]) and b["coef"] == 0.0


def test_grad_stats_guards_and_skipped_field(lib, vectors):
    """the record's `skipped` is not written; sentinels around the record and the workspace stay"""
    n = SPAN + 1
    g = vectors[n][0].to(DEV)
    rec, rbuf = _guarded(4, torch.int32, sentinel=-99)
    rec.copy_(torch.tensor([0, 0, 0, 41], dtype=torch.int32))
    nb = TS.grad_stats_workspace_bytes(n)
    wbuf = torch.full((nb + 2 * 256,), 0xEE, dtype=torch.uint8, device=DEV)
    a = _stats(lib, g, 1.0, 0.0, wbuf[256:256 + nb], rec)
    assert a["skipped"] == 41 and a["nonfinite"] == 0 and a["norm"] > 0
    assert _intact(rbuf, 4, sentinel=-99)
    assert bool((wbuf[:256] == 0xEE).all()) and bool((wbuf[256 + nb:] == 0xEE).all())


# ---------------------------------------------------------------------------------- 2, 3: grad_accumulate
@pytest.mark.parametrize("n", SIZES)
def test_grad_accumulate_is_the_left_to_right_fp32_sum(lib, vectors, n):
    h0, h1, h2 = vectors[n]
    acc, abuf = _guarded(n)
    gs = [_guarded(n) for _ in range(3)]
    for (g, _), h in zip(gs, (h0, h1, h2)):
        g.copy_(h)
    for i, (g, _) in enumerate(gs):
        _lib.check(lib.ishara_gradient_accumulate(None, _lib.ptr(acc), _lib.ptr(g), n, 1 if i == 0 else 0, _lib.stream()), "ishara_gradient_accumulate")
    assert torch.equal(acc.cpu(), (h0 + h1) + h2)           # acc held the sentinel before: first=1 overwrote it
    assert _intact(abuf, n)
    for (g, gbuf), h in zip(gs, (h0, h1, h2)):
        assert _intact(gbuf, n) and torch.equal(g.cpu(), h)


# ---------------------------------------------------------------------------------- models
KW = CFGS["tiny"]
LR = 4e-3


@pytest.fixture(scope="module")
def batches():
    from oracle import ishara_oracle as O
    ocfg = _oracle_cfg(KW, 0.0)
    return [O.synthetic_batch(ocfg, KW["B"], seed=s) for s in (2, 3, 4)]


def _slots(m):
    return [t.clone() for t in (m.params, m.opt_m, m.opt_v, m.opt_slow)]


def _trained(m):
    """the trainable prefix of params and the slots: what the optimizer writes (the BatchNorm statistics behind it are the forward's)"""
    return [m.params[:m.n_train].clone()] + [t.clone() for t in (m.opt_m, m.opt_v, m.opt_slow)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_legacy_identity(lib, batches):
    """ishara_optimizer_step, ishara_optimizer_step_ex(NULL, NULL, 0) and the record path with coef exactly 1.0 leave identical params and
    slots after each of 6 steps (the gradient of model A is copied into B and C, so only the update is compared)"""
    a, b, c = (_build(KW, "f32", 0.0) for _ in range(3))
    x, y = batches[0]
    rec = torch.zeros(4, dtype=torch.int32, device=DEV)
    ws = torch.empty(TS.grad_stats_workspace_bytes(c.n_train), dtype=torch.uint8, device=DEV)
    for step in range(6):
        a.loss_and_gradients(x, y, seed=step)
        b.grads.copy_(a.grads); c.grads.copy_(a.grads)
        _lib.check(lib.ishara_optimizer_step(a._h, F(LR), F(0.0), _lib.stream()))
        _lib.check(lib.ishara_optimizer_step_ex(b._h, F(LR), F(0.0), None, None, 0, _lib.stream()))
        _lib.check(lib.ishara_gradient_stats(c._h, _lib.ptr(c.grads), c.n_train, F(1.0), F(1e30), _lib.ptr(rec), _lib.ptr(ws), _lib.stream()))
        _lib.check(lib.ishara_optimizer_step_ex(c._h, F(LR), F(0.0), _lib.ptr(c.grads), _lib.ptr(rec), 1, _lib.stream()))
        assert np.frombuffer(rec.cpu().numpy().tobytes(), np.float32)[1] == 1.0
        sa = _trained(a)
        assert _same(sa, _trained(b)), f"step_ex(NULL, NULL, 0) differs at step {step + 1}"
        assert _same(sa, _trained(c)), f"coef == 1.0 differs at step {step + 1}"
    assert lib.ishara_optimizer_iterations(a._h) == lib.ishara_optimizer_iterations(b._h) == lib.ishara_optimizer_iterations(c._h) == 6


def test_clipped_steps_against_the_restated_algorithm(batches):
    from oracle import ishara_oracle as O
    model = _build(KW, "f32", 0.0)
    x, y = batches[0]
    nt = model.n_train
    theta = model.params[:nt].cpu().numpy().copy()
    st = O.optimizer_init(theta)
    model.optimizer.learning_rate = LR
    model.loss_and_gradients(x, y, seed=0)
    norm0 = float(np.sqrt(np.sum(model.grads[:nt].cpu().numpy().astype(np.float64) ** 2)))
    model.optimizer.global_clipnorm = clip = 0.5 * norm0
    coefs = []
    for step in range(6):
        model.train_on_batch(x, y, seed=step)
        g = model.grads[:nt].cpu().numpy().copy()
        got = model.grad_stats()
        ref_norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        want = TS.grad_stats_reference(g, 1.0, clip)
        print(f"step {step + 1}: norm {got['norm']!r} ref {ref_norm!r} coef {got['coef']!r} want {want['coef']!r}")
        assert _rel(got["norm"], ref_norm) <= 1e-6 and _rel(got["coef"], want["coef"]) <= 1e-6
        assert got["nonfinite"] == 0 and got["skipped"] == 0
        coefs.append(got["coef"])
        theta = O.optimizer_step(theta, g * np.float32(want["coef"]), st, lr=LR)
        err = np.abs(model.params[:nt].cpu().numpy() - theta).max()
        assert err <= 2e-6 * (1 + np.abs(theta).max()), f"step {step + 1}: {err:.3e}"
    assert min(coefs) < 1.0 and coefs[0] < 1.0
    assert model.optimizer.iterations == 6 and model._steps == 6


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_nonfinite_step_is_skipped(batches, bad):
    model = _build(KW, "f32", 0.0)
    x, y = batches[0]
    model.optimizer.learning_rate = LR
    model.optimizer.skip_nonfinite = True
    model.loss_and_gradients(x, y, seed=1)
    model.grads[model.n_train // 2] = bad                    # a memory write from torch; nothing faults
    before = _slots(model)                                   # after the forward: the BatchNorm statistics of this batch are in params
    model.apply_gradients()
    assert _same(before, _slots(model)), "a skipped step wrote to params or a slot"
    st = model.grad_stats()
    assert st["skipped"] == 1 and st["nonfinite"] == 1
    assert model.optimizer.iterations == 1 and model._lib.ishara_optimizer_iterations(model._h) == 1
    model.loss_and_gradients(x, y, seed=2)
    p0 = model.params.clone()
    model.apply_gradients()
    st = model.grad_stats()
    assert st["skipped"] == 1 and st["nonfinite"] == 0 and model.optimizer.iterations == 2
    assert not torch.equal(p0[:model.n_train], model.params[:model.n_train]) and bool(torch.isfinite(model.params).all())


def test_nonfinite_without_the_guard_is_todays_step(batches):
    """skip_nonfinite=False and no clipping: the record is not consulted (and never allocated); the call succeeds"""
    model = _build(KW, "f32", 0.0)
    x, y = batches[0]
    model.loss_and_gradients(x, y, seed=1)
    model.grads[3] = float("nan")
    model.apply_gradients()
    torch.cuda.synchronize()
    assert model._gstats is None and model.optimizer.iterations == 1


def _record_seeds(model, monkeypatch):
    seen = []
    orig = model.loss_and_gradients

    def spy(x, y, seed=None, loss_scale=1.0):
        seen.append((seed, loss_scale))
        return orig(x, y, seed=seed, loss_scale=loss_scale)
    monkeypatch.setattr(model, "loss_and_gradients", spy)
    return seen


def test_accumulation(batches):
    from oracle import ishara_oracle as O
    model = _build(KW, "f32", 0.0)
    nt = model.n_train
    model.optimizer.learning_rate = LR
    model.optimizer.accumulate_steps = 2
    theta = model.params[:nt].cpu().numpy().copy()
    st = O.optimizer_init(theta)
    snaps = []
    for j, (x, y) in enumerate(batches[:2]):
        model.train_on_batch(x, y, seed=11 + j)
        snaps.append(model.grads[:nt].clone())
        assert model.optimizer.iterations == j and model._steps == j      # 0 after the first microbatch, 1 after the cycle
    assert not torch.equal(snaps[0], snaps[1])
    assert torch.equal(model._grad_acc, snaps[0] + snaps[1])
    got = model.grad_stats()
    gsum = (snaps[0] + snaps[1]).cpu().numpy()
    assert got["coef"] == 0.5 and _rel(got["norm"], 0.5 * float(np.sqrt(np.sum(gsum.astype(np.float64) ** 2)))) <= 1e-6
    theta = O.optimizer_step(theta, gsum * np.float32(0.5), st, lr=LR)
    err = np.abs(model.params[:nt].cpu().numpy() - theta).max()
    assert err <= 2e-6 * (1 + np.abs(theta).max()), f"{err:.3e}"
    assert model.optimizer.iterations == 1 and model._micro == 0


def test_accumulation_seeds(batches, monkeypatch):
    """without explicit seeds microbatch j of cycle c draws from seed index c * k + j: the masks of two microbatches differ, and with
    accumulate_steps = 1 the seeds are today's (index = the step count)"""
    model = _build(KW, "bf16", 0.2)
    x, y = batches[0]
    model.optimizer.accumulate_steps = 2
    seen = _record_seeds(model, monkeypatch)
    grads = []
    for _ in range(4):
        model.train_on_batch(x, y)
        grads.append(model.grads[:model.n_train].clone())
    assert not torch.equal(grads[0], grads[1])               # the same batch, the same weights, other dropout masks
    assert [s for s, _ in seen] == [(model._step_seed + 0x9E3779B1 * i) & 0xFFFFFFFF for i in range(4)]
    assert model.optimizer.iterations == 2
    one = _build(KW, "bf16", 0.2)
    one.optimizer.global_clipnorm = 1e30                     # the new path with k = 1
    seen = _record_seeds(one, monkeypatch)
    for _ in range(3):
        one.train_on_batch(x, y)
    assert [s for s, _ in seen] == [(one._step_seed + 0x9E3779B1 * i) & 0xFFFFFFFF for i in range(3)]


def test_data_parallel_order(batches, monkeypatch):
    """world = 2 rehearsed on one GPU: one all-reduce per cycle, of the accumulator, in front of the statistics; loss_scale = 1/2"""
    from ishara_amd import parallel
    model = _build(KW, "f32", 0.0)
    model.optimizer.accumulate_steps = 2
    model.optimizer.global_clipnorm = 1.0
    events = []
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    monkeypatch.setattr(parallel, "allreduce_sum_", lambda t: (events.append(("allreduce", t.data_ptr(), t.numel())), t)[1])
    orig = model._launch_grad_stats
    monkeypatch.setattr(model, "_launch_grad_stats", lambda src, scale, clip: (events.append(("grad_stats", src.data_ptr(), scale)), orig(src, scale, clip))[1])
    seen = _record_seeds(model, monkeypatch)
    for x, y in batches[:2]:
        model.train_on_batch(x, y, seed=5)
    torch.cuda.synchronize()
    assert events == [("allreduce", model._grad_acc.data_ptr(), model.n_train), ("grad_stats", model._grad_acc.data_ptr(), 0.5)]
    assert [ls for _, ls in seen] == [0.5, 0.5]
    assert model.optimizer.iterations == 1


def _fresh(seed, clip=2.0):
    m = _build(KW, "bf16", 0.2, seed=seed)
    m.optimizer.learning_rate = LR
    m.optimizer.global_clipnorm = clip
    return m


def test_load_state_restores_every_bit(batches, tmp_path):
    """save_state after 3 steps, load_state into a model built from another seed: params (BatchNorm statistics included), the three
    slots, the counters and the settings are the saved run's; in the middle of a cycle the state is refused"""
    b = _fresh(3)
    for i in range(3):
        b.train_on_batch(*batches[i % 3])
    path = b.save_state(str(tmp_path / "state"))
    c = _fresh(99, clip=None)
    assert not torch.equal(c.params, b.params)
    c.load_state(path)
    assert _same(_slots(b), _slots(c))
    assert c.optimizer.global_clipnorm == 2.0 and c.optimizer.iterations == 3 and c._steps == 3 and c._step_seed == b._step_seed
    assert c._lib.ishara_optimizer_iterations(c._h) == 3 and float(c.optimizer.learning_rate) == LR
    assert c.optimizer.train_options() == b.optimizer.train_options()
    c.optimizer.accumulate_steps = 2
    c.train_on_batch(*batches[0])
    with pytest.raises(ValueError, match="middle of an accumulation cycle"):
        c.save_state(str(tmp_path / "mid"))


def test_resume_is_bit_identical(batches, tmp_path):
    """Run A trains 6 steps; run B trains 3, saves, a model built from another seed loads and trains 3 more on the same batches: params,
    BatchNorm statistics and slots bit-identical (bf16, dropout 0.2, global_clipnorm set, default seeds).

    The test needs a training step that repeats bit for bit between two model objects.  It did not at this shape while the generic
    depthwise-conv weight gradient (this model's width-7 Conformer convolution) summed through global float atomics: two models built
    alike differed after ONE step of the default path (max |difference| of `grads` 2.4e-7, of opt_m 3.0e-8), and the resumed run left
    the uninterrupted one by params 5.2e-10 .. 3.7e-9, opt_m 1.9e-9, opt_v 9.1e-13 .. 1.8e-12, opt_slow 1.5e-10 after steps 4 - 6, although
    load_state had restored every bit (test_load_state_restores_every_bit).  That kernel now writes partial rows that are summed in a
    fixed order (csrc/dwconv_bwd.hip, dwconv_wgrad_kernel)."""
    a = _fresh(3)
    for i in range(6):
        a.train_on_batch(*batches[i % 3])
    b = _fresh(3)
    for i in range(3):
        b.train_on_batch(*batches[i % 3])
    path = b.save_state(str(tmp_path / "state"))
    c = _fresh(99)
    c.load_state(path)
    for i in range(3, 6):
        c.train_on_batch(*batches[i % 3])
    for name, x, y in zip(("params", "opt_m", "opt_v", "opt_slow"), _slots(a), _slots(c)):
        print(f"resume: max |A - B| of {name}: {float((x - y).abs().max()):.3e}")
    assert _same(_slots(a), _slots(c)), "the resumed run left the uninterrupted one"
    assert c.grad_stats()["norm"] == a.grad_stats()["norm"]


def test_fit_logs_initial_epoch_and_checkpoint(batches, tmp_path):
    from ishara_amd import LearningRateScheduler
    from ishara_amd.evaluation import TrainStateCheckpoint
    model = _build(KW, "bf16", 0.2)
    h = model.fit(batches, epochs=1, verbose=0)
    assert "grad_norm" not in h.history and "skipped_steps" not in h.history
    model.optimizer.global_clipnorm = 1.0
    seen = []
    ck = TrainStateCheckpoint(str(tmp_path / "ck_{epoch}"), every_epochs=2)
    h = model.fit(batches, epochs=3, initial_epoch=1, verbose=0, callbacks=[LearningRateScheduler(lambda e: (seen.append(e), LR)[1]), ck])
    assert seen == [1, 2] and h.epoch == [1, 2]
    assert len(h.history["grad_norm"]) == 2 and np.isfinite(h.history["grad_norm"]).all() and min(h.history["grad_norm"]) > 0
    assert h.history["skipped_steps"] == [0, 0]
    assert model.optimizer.iterations == 9
    assert ck.last_path == str(tmp_path / "ck_2.npz")
    other = _build(KW, "bf16", 0.2, seed=99)
    other.load_state(ck.last_path)
    assert other.optimizer.iterations == 6 and other.optimizer.global_clipnorm == 1.0       # written at the end of epoch index 1


def test_graph_capture_replays_the_eager_cycle(lib, batches):
    """grad_stats + optimizer_step_ex captured on one stream (no side stream, so no parallel branches) replay to the eager result"""
    model = _build(KW, "f32", 0.0)
    x, y = batches[0]
    model.optimizer.learning_rate = LR
    model.loss_and_gradients(x, y, seed=1)
    src = model.grads[:model.n_train]
    before = _slots(model)

    def cycle():
        model._launch_grad_stats(src, 1.0, 0.01)
        model._apply_gradients_ex(src, True)
    cycle()                                                  # eager (also loads the kernels before the capture)
    torch.cuda.synchronize()
    eager, eager_rec = _slots(model), model._gstats.clone()
    assert not torch.equal(eager[0], before[0])

    def rewind():
        for t, s in zip((model.params, model.opt_m, model.opt_v, model.opt_slow), before):
            t.copy_(s)
        model._gstats.zero_()
        _lib.check(lib.ishara_optimizer_set_iterations(model._h, 0))
    rewind()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cycle()
    rewind()                                                 # the capture ran nothing, but consumed an iteration number on the host
    graph.replay()
    torch.cuda.synchronize()
    assert _same(eager, _slots(model)) and torch.equal(eager_rec, model._gstats)
