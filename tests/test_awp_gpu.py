"""GPU: adversarial weight perturbation, from the kernels of csrc/awp.hip (against train_state.awp_reference on the tables, vectors and
variants of awp_parity.py, with guard elements on both sides of every buffer the call writes) to Model: train_on_batch on both step
paths against the same step composed from the public pieces, the option switched off or not yet started, the direction of the step,
skipped steps, accumulation cycles, the order of a two-rank cycle, save_state / load_state, the moving average and graph capture.  The
model tests use CFGS["tiny"] of test_model_gpu.py.

The comparison (awp_parity.compare; tests/test_awp_mutants.py shows it rejecting the ordinary mistakes): scale within 1 fp32 ulp of the
reference's, the perturbed weights bit for bit fp32(w + fp32(scale * g)) from the device's own scale, the copy and the gradient bit for
bit, the two counts exactly, the two norms within 1e-6 relative.  Model against composition is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import awp_parity as AP
from ishara_amd import _lib, train_state as TS
from test_model_gpu import CFGS, _build, _oracle_cfg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
F = C.c_float


def _guarded(n, dtype=torch.float32, sentinel=-7.5, shift=0):
    """a [n] view with GUARD (+ shift) sentinel elements in front and GUARD behind -> (view, whole buffer); shift = 0: 16-byte aligned"""
    buf = torch.full((n + 2 * GUARD + shift,), sentinel, dtype=dtype, device=DEV)
    return buf[GUARD + shift:GUARD + shift + n], buf


def _intact(buf, n, sentinel=-7.5, shift=0):
    return bool((buf[:GUARD + shift] == sentinel).all()) and bool((buf[GUARD + shift + n:] == sentinel).all())


class _Case:
    """the device buffers of one awp_parity case, each between guards; g_shift = 1 puts g on a 4-byte boundary only"""

    def __init__(self, lib, name, variant="plain", relative=False, g_shift=0):
        self.lib, self.key, self.relative, self.g_shift = lib, (name, variant, relative), relative, g_shift
        seg = AP.table(name)
        self.n, self.S = int(seg[-1]), len(seg) - 1
        self.w0, self.g0 = AP.vectors(name, variant)
        self.seg = torch.from_numpy(np.array(seg)).to(DEV)
        self.w, self.w_buf = _guarded(self.n)
        self.backup, self.backup_buf = _guarded(self.n)
        self.g, self.g_buf = _guarded(self.n, shift=g_shift)
        self.scale, self.scale_buf = _guarded(self.S)
        self.rec, self.rec_buf = _guarded(4, torch.int32, sentinel=-99)
        self.ws_bytes = int(lib.ishara_awp_workspace_bytes(self.n, self.S))
        assert self.ws_bytes > 0
        self.ws, self.ws_buf = _guarded(self.ws_bytes, torch.uint8, sentinel=0xA5)
        self.load()

    def load(self):
        self.w.copy_(torch.from_numpy(self.w0.copy()))
        self.g.copy_(torch.from_numpy(self.g0.copy()))

    def perturb(self):
        assert self.g.data_ptr() % 16 == (4 * self.g_shift) % 16 and self.w.data_ptr() % 16 == 0 and self.backup.data_ptr() % 16 == 0
        _lib.check(self.lib.ishara_awp_perturb(None, _lib.ptr(self.w), _lib.ptr(self.backup), _lib.ptr(self.g), _lib.ptr(self.seg), self.S, self.n,
                                               F(AP.DELTA), F(AP.EPS), 1 if self.relative else 0, _lib.ptr(self.scale), _lib.ptr(self.rec),
                                               _lib.ptr(self.ws), _lib.stream()), "ishara_awp_perturb")
        torch.cuda.synchronize()
        raw = self.rec.cpu().numpy()
        stats = dict(grad_norm=float(raw[:2].view(np.float32)[0]), delta_norm=float(raw[:2].view(np.float32)[1]), perturbed=int(raw[2]), zeroed=int(raw[3]))
        return dict(w_adv=self.w.cpu().numpy(), backup=self.backup.cpu().numpy(), g_after=self.g.cpu().numpy(), scale=self.scale.cpu().numpy(), stats=stats)

    def restore(self):
        _lib.check(self.lib.ishara_awp_restore(None, _lib.ptr(self.w), _lib.ptr(self.backup), self.n, _lib.stream()), "ishara_awp_restore")
        torch.cuda.synchronize()

    def intact(self):
        return (_intact(self.w_buf, self.n) and _intact(self.backup_buf, self.n) and _intact(self.g_buf, self.n, shift=self.g_shift)
                and _intact(self.scale_buf, self.S) and _intact(self.rec_buf, 4, -99) and _intact(self.ws_buf, self.ws_bytes, 0xA5))


def _bytes(got):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else repr(sorted(v.items()))) for k, v in got.items()}


# ---------------------------------------------------------------------------------- 1: the kernel against the reference
@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_perturb_equals_the_reference(lib, name, relative):
    c = _Case(lib, name, "plain", relative)
    got = c.perturb()
    assert AP.compare(got, name, "plain", relative) == []
    assert c.intact()
    c.load()                                                   # a second run: the same bits (fixed-order sums, no atomics)
    assert _bytes(c.perturb()) == _bytes(got)
    assert c.intact()


@pytest.mark.parametrize("variant", ["plain", "nonfinite"])
def test_perturb_with_a_gradient_on_a_4_byte_boundary(lib, variant):
    """g is only required to be a float array: off a 16-byte boundary the kernels read it element by element"""
    c = _Case(lib, "A", variant, g_shift=1)
    assert AP.compare(c.perturb(), "A", variant) == []
    assert c.intact()


# ---------------------------------------------------------------------------------- 2: zero-gradient, NaN, Inf and 3e19 segments
@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_zero_nan_inf_and_huge_segments(lib, name, relative):
    seg = AP.table(name)
    zs, ns, fs, hs = AP.variant_segments(seg)
    plain = _Case(lib, name, "plain", relative).perturb()
    span = lambda a, s: a[seg[s]:seg[s + 1]].tobytes()      # noqa: E731
    others = lambda a, skip: b"".join(span(a, s) for s in range(len(seg) - 1) if s not in skip)      # noqa: E731

    c = _Case(lib, name, "nonfinite", relative)
    got = c.perturb()
    assert AP.compare(got, name, "nonfinite", relative) == [] and c.intact()
    assert got["stats"]["zeroed"] == len({ns, fs}) and got["stats"]["perturbed"] == len(seg) - 1 - len({ns, fs})
    for s in {ns, fs}:
        assert got["scale"][s] == 0 and span(got["w_adv"], s) == span(c.w0, s)
    assert others(got["w_adv"], {ns, fs}) == others(plain["w_adv"], {ns, fs})      # the other segments do not see the NaN and the Inf
    assert np.array_equal(np.delete(got["scale"], list({ns, fs})), np.delete(plain["scale"], list({ns, fs})))
    assert np.isfinite(got["stats"]["grad_norm"]) and np.isfinite(got["stats"]["delta_norm"])

    c = _Case(lib, name, "zero_grad", relative)
    got = c.perturb()
    assert AP.compare(got, name, "zero_grad", relative) == [] and c.intact()
    assert got["stats"]["zeroed"] == 0 and np.isfinite(got["scale"][zs]) and span(got["w_adv"], zs) == span(c.w0, zs)      # a finite scale, a step of 0
    assert others(got["w_adv"], {zs}) == others(plain["w_adv"], {zs})

    c = _Case(lib, name, "huge", relative)
    got = c.perturb()
    assert AP.compare(got, name, "huge", relative) == [] and c.intact()
    assert got["stats"]["zeroed"] == 0 and got["scale"][hs] > 0 and span(got["w_adv"], hs) != span(c.w0, hs)      # ss_g stays finite in fp64
    assert others(got["w_adv"], {hs}) == others(plain["w_adv"], {hs})


# ---------------------------------------------------------------------------------- 3: the restore
@pytest.mark.parametrize("name,variant", [("A", "plain"), ("A", "nonfinite"), ("B", "plain"), ("C", "huge")])
def test_restore_puts_every_bit_back(lib, name, variant):
    c = _Case(lib, name, variant)
    got = c.perturb()
    assert got["w_adv"].tobytes() != c.w0.tobytes()
    c.restore()
    assert c.w.cpu().numpy().tobytes() == c.w0.tobytes() and c.intact()


def test_restore_keeps_nan_payloads(lib):
    """weights of random 32-bit words (NaNs with payloads, signalling NaNs, infinities, subnormals): the perturbation computes on them,
    the copy and the restore move words"""
    c = _Case(lib, "A")
    words = np.random.default_rng(5).integers(0, 2 ** 32, size=c.n, dtype=np.uint32)
    words[:6] = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff80abcd, 0x7f800000, 0x00000001], dtype=np.uint32)
    c.w.view(torch.int32).copy_(torch.from_numpy(words.view(np.int32).copy()))
    got = c.perturb()
    assert got["backup"].view(np.uint32).tobytes() == words.tobytes()
    assert got["w_adv"].view(np.uint32).tobytes() != words.tobytes() and got["stats"]["zeroed"] == 0
    c.restore()
    assert c.w.cpu().numpy().view(np.uint32).tobytes() == words.tobytes() and c.intact()


# ---------------------------------------------------------------------------------- models
KW = CFGS["tiny"]
LR = 4e-3
DELTA = 0.2


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


class _Pieces:
    """the AWP (micro)batch of a twin model from the public pieces: loss_and_gradients, the raw ishara_awp_perturb, ishara_sync_weights,
    loss_and_gradients with the same seed, ishara_awp_restore (and ishara_sync_weights again when no optimizer step follows)"""

    def __init__(self, m, delta=DELTA, eps=1e-4, relative=False):
        self.m, self.delta, self.eps, self.relative = m, delta, eps, relative
        seg = TS.awp_segments(m.entries, m.n_train)
        self.S = len(seg) - 1
        self.seg = torch.from_numpy(seg).to(DEV)
        self.backup = torch.empty(m.n_train, dtype=torch.float32, device=DEV)
        self.scale = torch.zeros(self.S, dtype=torch.float32, device=DEV)
        self.rec = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.ws = torch.empty(int(m._lib.ishara_awp_workspace_bytes(m.n_train, self.S)), dtype=torch.uint8, device=DEV)

    def perturb(self):
        m = self.m
        _lib.check(m._lib.ishara_awp_perturb(m._h, _lib.ptr(m.params), _lib.ptr(self.backup), _lib.ptr(m.grads), _lib.ptr(self.seg), self.S, m.n_train,
                                             F(self.delta), F(self.eps), 1 if self.relative else 0, _lib.ptr(self.scale), _lib.ptr(self.rec),
                                             _lib.ptr(self.ws), _lib.stream()), "ishara_awp_perturb")
        _lib.check(m._lib.ishara_sync_weights(m._h, _lib.stream()), "ishara_sync_weights")

    def restore(self, sync=False):
        m = self.m
        _lib.check(m._lib.ishara_awp_restore(m._h, _lib.ptr(m.params), _lib.ptr(self.backup), m.n_train, _lib.stream()), "ishara_awp_restore")
        if sync:
            _lib.check(m._lib.ishara_sync_weights(m._h, _lib.stream()), "ishara_sync_weights")

    def gradient(self, x, y, seed, loss_scale=1.0, sync=False):
        """-> (clean loss, adversarial loss) as floats' tensors; m.grads hold the second gradient"""
        m = self.m
        clean = m.loss_and_gradients(x, y, seed=seed)[0].clone()
        self.perturb()
        adv = m.loss_and_gradients(x, y, seed=seed, loss_scale=loss_scale)[0].clone()
        self.restore(sync)
        return clean, adv


@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_step_equals_the_composition(batches, dtype, relative):
    """4: three steps, dropout 0.2.  bf16 reads the 16-bit weight shadows: equal bits prove they were refreshed behind the perturbation"""
    a = _model(dtype, 0.2, awp_delta=DELTA, awp_relative=relative)
    twin = _model(dtype, 0.2)
    plain = _model(dtype, 0.2)
    pieces = _Pieces(twin, relative=relative)
    for step in range(3):
        x, y = batches[step]
        loss = a.train_on_batch(x, y, seed=step)
        before = twin.params[:twin.n_train].clone()
        clean, adv = pieces.gradient(x, y, step)
        assert torch.equal(twin.params[:twin.n_train], before)                   # the restore is exact
        twin.apply_gradients()
        plain.train_on_batch(x, y, seed=step)
        assert _same(_slots(a), _slots(twin)), f"step {step + 1}: train_on_batch left the composition"
        assert torch.equal(loss, clean)
        st = a.awp_stats()
        assert st["clean_loss"] == float(clean.item()) and st["adv_loss"] == float(adv.item())
        assert st["perturbed"] == pieces.S and st["zeroed"] == 0 and st["grad_norm"] > 0 and st["delta_norm"] > 0
        assert torch.equal(a._awp["scale"], pieces.scale) and torch.equal(a._awp["rec"], pieces.rec)
    assert a.optimizer.iterations == 3 and a._steps == 3
    assert not torch.equal(a.params, plain.params), "the perturbation changed nothing"
    scales = a.awp_scales()
    assert list(scales) == [n for n, _, _, t in a.entries if t] and all(v > 0 for v in scales.values())
    assert a._gstats is None                                   # the default step path: no grad-stats record was needed


def test_scales_follow_the_reference_on_the_model_gradient(batches):
    m = _model("f32", 0.0, awp_delta=DELTA)
    x, y = batches[0]
    m.loss_and_gradients(x, y, seed=1)
    w, g = m.params[:m.n_train].cpu().numpy(), m.grads[:m.n_train].cpu().numpy()
    _, scale, stats = TS.awp_reference(w, g, TS.awp_segments(m.entries, m.n_train), DELTA, 1e-4)
    m.train_on_batch(x, y, seed=1)
    got = np.array(list(m.awp_scales().values()), np.float32)
    assert AP.ulps(got, scale).max() <= 1
    st = m.awp_stats()
    assert abs(st["grad_norm"] - stats["grad_norm"]) <= 1e-6 * stats["grad_norm"] and abs(st["delta_norm"] - stats["delta_norm"]) <= 1e-6 * stats["delta_norm"]


# ---------------------------------------------------------------------------------- 5: off, and not started yet
def test_off_and_not_started_are_the_plain_step(batches):
    base = _model("bf16", 0.2)
    off = _model("bf16", 0.2, awp_delta=None, awp_eps=1e-3, awp_relative=True)
    late = _model("bf16", 0.2, awp_delta=DELTA, awp_start_step=3)
    two = _model("bf16", 0.2, awp_delta=DELTA, awp_start_step=2)
    for step in range(3):
        for m in (base, off, late, two):
            m.train_on_batch(*batches[step], seed=step)
        assert _same(_slots(base), _slots(off)) and _same(_slots(base), _slots(late)), step
        assert _same(_slots(base), _slots(two)) == (step < 2), step              # steps 0 and 1 are plain, step 2 is perturbed
        assert (two._awp_backup is None) == (step < 2)
    for m in (off, late):
        assert m._awp_backup is None and m._awp is None
        with pytest.raises(_lib.IsharaError, match="no step has run"):
            m.awp_stats()
    late.train_on_batch(*batches[0], seed=3)                   # iterations == 3: started
    assert late._awp_backup is not None and late.awp_stats()["perturbed"] > 0


def test_profiler_keys(batches):
    m = _model("bf16", 0.0)
    prof = m.profile_step(*batches[0])
    assert not any(k.startswith("awp_") for k in prof)
    m.optimizer.awp_delta = DELTA
    prof = m.profile_step(*batches[0])
    n = m.n_train
    assert {k: (prof[k]["launches"], prof[k]["bytes"]) for k in ("awp_norms", "awp_perturb", "awp_restore")} == \
        {"awp_norms": (1, 4.0 * n), "awp_perturb": (1, 16.0 * n), "awp_restore": (1, 8.0 * n)}
    m.optimizer.awp_relative = True
    assert m.profile_step(*batches[0])["awp_norms"]["bytes"] == 8.0 * n


# ---------------------------------------------------------------------------------- 6: the direction
def test_the_perturbation_raises_the_loss(batches):
    """f32, dropout 0, awp_delta = 0.01, the batch of seed 2 (batches[0]), dropout seed 0, weights of seed 3.  Chosen on the CPU with
    oracle/ishara_oracle.py alone: the CTC loss at these weights is 165.28017, at the weights train_state.awp_reference perturbs by the
    oracle's own gradient 168.91902: an increase of 3.64, against an fp32 loss error of the model below 2e-3 (1e-5 relative)."""
    m = _model("f32", 0.0, awp_delta=0.01)
    loss = m.train_on_batch(*batches[0], seed=0)
    st = m.awp_stats()
    assert st["clean_loss"] == float(loss.item())
    assert abs(st["clean_loss"] - 165.28017) < 2e-2 and abs(st["adv_loss"] - 168.91902) < 2e-2
    assert st["adv_loss"] > st["clean_loss"] + 3.0


# ---------------------------------------------------------------------------------- 7: skipped steps
def test_skipped_step_leaves_the_weights_bit_for_bit(batches):
    m = _model("f32", 0.0, awp_delta=DELTA, skip_nonfinite=True)
    x, y = batches[0]
    m.train_on_batch(x, y, seed=0)
    theta = m.params[:m.n_train].clone()
    m._loss_and_gradients_step(x, y, 1, 1.0, None)             # both passes, the perturbation and the restore
    assert torch.equal(m.params[:m.n_train], theta)
    m.grads[m.n_train // 2] = float("nan")                     # a memory write from torch; nothing faults
    before = _slots(m)
    m.apply_gradients()
    assert _same(before, _slots(m)) and torch.equal(m.params[:m.n_train], theta), "a skipped step wrote to params or a slot"
    gs = m.grad_stats()
    assert gs["skipped"] == 1 and gs["nonfinite"] == 1 and m.optimizer.iterations == 2
    m.train_on_batch(x, y, seed=2)
    assert m.grad_stats()["skipped"] == 1 and not torch.equal(m.params[:m.n_train], theta)


def test_nan_in_the_first_gradient_zeroes_one_tensor(batches, monkeypatch):
    m = _model("f32", 0.0, awp_delta=DELTA, skip_nonfinite=True)
    x, y = batches[0]
    names = [n for n, _, _, t in m.entries if t]
    victim = names[len(names) // 2]
    off = {n: o for n, _, o, _ in m.entries}[victim]
    orig, calls = m.loss_and_gradients, []

    def poisoned(x, y, seed=None, loss_scale=1.0):
        out = orig(x, y, seed=seed, loss_scale=loss_scale)
        calls.append(loss_scale)
        if len(calls) == 1:
            m.grads[off] = float("nan")                        # into the pass-1 gradient only: pass 2 rewrites grads
        return out
    monkeypatch.setattr(m, "loss_and_gradients", poisoned)
    theta = m.params[:m.n_train].clone()
    m.train_on_batch(x, y, seed=0)
    scales, st = m.awp_scales(), m.awp_stats()
    assert scales[victim] == 0.0 and all(v > 0 for n, v in scales.items() if n != victim)
    assert st["zeroed"] == 1 and st["perturbed"] == len(names) - 1 and np.isfinite(st["grad_norm"]) and np.isfinite(st["adv_loss"])
    assert m.grad_stats()["skipped"] == 0 and not torch.equal(m.params[:m.n_train], theta)      # the second gradient is finite: the step is applied
    assert bool(torch.isfinite(m.params).all())


# ---------------------------------------------------------------------------------- 8: accumulation
def test_accumulation_cycle_equals_the_composition(batches):
    a = _model("bf16", 0.2, awp_delta=DELTA, accumulate_steps=2, global_clipnorm=1.0)
    twin = _model("bf16", 0.2, global_clipnorm=1.0)
    pieces = _Pieces(twin)
    acc = torch.empty(twin.n_train, dtype=torch.float32, device=DEV)
    for cycle in range(2):
        for j in range(2):
            x, y = batches[(2 * cycle + j) % 3]
            seed = 10 * cycle + j
            loss = a.train_on_batch(x, y, seed=seed)
            clean, _ = pieces.gradient(x, y, seed, sync=(j == 0))
            assert torch.equal(loss, clean)
            _lib.check(twin._lib.ishara_gradient_accumulate(twin._h, _lib.ptr(acc), _lib.ptr(twin.grads), twin.n_train, 1 if j == 0 else 0, _lib.stream()),
                       "ishara_gradient_accumulate")
            if j == 0:
                assert torch.equal(a.params[:a.n_train], twin.params[:twin.n_train]) and a.optimizer.iterations == cycle
        twin._launch_grad_stats(acc, 0.5, 1.0)
        twin._apply_gradients_ex(acc, False)
        assert _same(_slots(a), _slots(twin)), f"cycle {cycle + 1}"
        assert torch.equal(a(batches[0][0]), twin(batches[0][0]))                # and the weight shadows
    assert a.optimizer.iterations == 2 and a._micro == 0


# ---------------------------------------------------------------------------------- 9: two ranks, rehearsed
@pytest.mark.parametrize("k", [1, 2])
def test_data_parallel_order(batches, monkeypatch, k):
    """world = 2 rehearsed on one GPU: no collective in pass 1, one all-reduce per cycle behind the last pass 2, loss scales 1 and 1/2"""
    from ishara_amd import parallel
    m = _model("f32", 0.0, awp_delta=DELTA, accumulate_steps=k, global_clipnorm=1.0 if k > 1 else None)
    events = []
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    monkeypatch.setattr(parallel, "overlap_enabled", lambda: False)
    monkeypatch.setattr(parallel, "allreduce_sum_", lambda t: (events.append(("allreduce", t.data_ptr(), t.numel())), t)[1])
    orig = m.loss_and_gradients

    def spy(x, y, seed=None, loss_scale=1.0):
        events.append(("pass", seed, loss_scale))
        return orig(x, y, seed=seed, loss_scale=loss_scale)
    monkeypatch.setattr(m, "loss_and_gradients", spy)
    for j in range(k):
        m.train_on_batch(*batches[j], seed=5 + j)
    torch.cuda.synchronize()
    src = m._grad_acc if k > 1 else m.grads
    want = [e for j in range(k) for e in (("pass", 5 + j, 1.0), ("pass", 5 + j, 0.5))] + [("allreduce", src.data_ptr(), m.n_train)]
    assert events == want
    assert m.optimizer.iterations == 1


# ---------------------------------------------------------------------------------- 10: state and the moving average
def _resumable(seed, awp=True):
    m = _build(KW, "bf16", 0.2, seed=seed)
    o = m.optimizer
    o.learning_rate, o.global_clipnorm = LR, 2.0
    o.use_ema, o.ema_momentum = True, 0.9
    if awp:
        o.awp_delta, o.awp_eps, o.awp_start_step, o.awp_relative = 0.15, 1e-3, 1, True
    return m


def test_resume_is_bit_identical_and_the_average_follows(batches, tmp_path):
    a = _resumable(3)
    avg, st = a.params[:a.n_train].cpu().numpy().copy(), TS.ema_state_init()
    for i in range(4):
        a.train_on_batch(*batches[i % 3])
        avg, _ = TS.ema_reference(avg, a.params[:a.n_train].cpu().numpy(), st, 0.9)      # the average of the restored-then-stepped weights
        assert a._ema_avg.cpu().numpy().tobytes() == avg.tobytes(), i
    b = _resumable(3)
    for i in range(2):
        b.train_on_batch(*batches[i % 3])
    path = b.save_state(str(tmp_path / "state"))
    with np.load(path) as z:
        assert set(z.files) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.EMA_KEYS + TS.AWP_KEYS)
    c = _resumable(99, awp=False)
    c.load_state(path)
    assert c.optimizer.awp_options() == b.optimizer.awp_options() == (0.15, 1e-3, 1, True)
    for i in range(2, 4):
        c.train_on_batch(*batches[i % 3])
    assert _same(_slots(a), _slots(c)), "the resumed run left the uninterrupted one"
    assert torch.equal(a._ema_avg, c._ema_avg) and a.awp_stats() == c.awp_stats()
    with a.averaged_weights():
        with pytest.raises(_lib.IsharaError, match="inside averaged_weights"):
            a.train_on_batch(*batches[0])
    plain = _resumable(3, awp=False)                            # a state without AWP has the keys it had, and leaves the options alone
    plain.train_on_batch(*batches[0])
    with np.load(plain.save_state(str(tmp_path / "plain"))) as z:
        assert set(z.files) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.EMA_KEYS)
    c.load_state(str(tmp_path / "plain"))
    assert c.optimizer.awp_options() == (0.15, 1e-3, 1, True)


# ---------------------------------------------------------------------------------- 11: graph capture
def test_graph_capture_replays_the_eager_bits(lib, batches):
    """perturb -> weight shadows -> a copy of the perturbed weights -> restore, one stream, a linear chain"""
    m = _model("f32", 0.0)
    x, y = batches[0]
    m.loss_and_gradients(x, y, seed=1)
    p = _Pieces(m)
    adv = torch.zeros(m.n_train, dtype=torch.float32, device=DEV)
    theta = m.params.clone()

    def chain():
        p.perturb()
        adv.copy_(m.params[:m.n_train])
        p.restore(sync=True)
    chain()                                                    # eager (also loads the kernels before the capture)
    torch.cuda.synchronize()
    eager = [t.clone() for t in (adv, p.backup, p.scale, p.rec, m.params)]
    assert torch.equal(m.params, theta) and not torch.equal(adv, theta[:m.n_train]) and torch.equal(p.backup, theta[:m.n_train])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for t in (adv, p.backup, p.scale):
        t.fill_(-3.0)
    p.rec.zero_()
    p.ws.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(e, t) for e, t in zip(eager, (adv, p.backup, p.scale, p.rec, m.params)))
