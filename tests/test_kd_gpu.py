"""GPU: ishara_kd_grad (csrc/kd_grad.hip), ishara_loss_backward_kd (csrc/keras_hybrid.hip) and the Python surface of knowledge distillation
(ishara_amd/kd.py, model.py).  Cases, bounds, the fp64 reference and the float32 twin are tests/kd_parity.py's.

   1  every case of the table within the bound of the fp64 reference: dlogits (accumulate 0 and 1) and kl_frame; none is skipped
   2  teacher = logits (the same pointer, and a copy): G == 0 and kl_frame == 0 exactly; accumulate 1 leaves dlogits equal to its old value
   3  accumulate 1 is float32(old + G0) bit for bit, G0 from an accumulate 0 run
   4  dlb is the round-to-nearest-even bf16 of the downloaded final rows, zero padded, bit for bit
   5  rows past a clip's end hold NaN in both inputs: +0 with accumulate 0, untouched with accumulate 1
   6  two runs are bit-identical
   7  kl_clip is the ascending float32 sum of the downloaded kl_frame, bit for bit
   8  every refusal fires before a launch
   9  a captured graph replays the call
  10  the whole model against the oracle in float64, f32 and bf16, both modes, with a fixed random teacher
  11  ishara_loss_backward_kd with teacher = the step's logits equals ishara_loss_backward_ex, and with the n-best stage
      ishara_loss_backward_nbest, element for element
  12  train_on_batch with a teacher: finite gradients under accumulation, clipping with skipping, AWP and MWER; the teacher runs once per
      microbatch
  13  kd_stats is the reference on the downloaded logits
  14  the option off: a step bit-equal to an optimizer built without the options, nothing allocated
  15  kd_loss on a ConformerEncoder output equals kd_grad by hand"""
import ctypes as C

import numpy as np
import pytest
import torch

import kd_parity as P
from ishara_amd import _lib, get_model, kd, mwer

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in P.cases()}


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # a copy: the cases' arrays are read-only


def _run(case, old=None, teacher="own", want_dlb=True):
    """one ishara_kd_grad call on a case -> dict of numpy arrays (dlogits, dlb uint32 [B * T, 64], kl_frame, kl_clip).  old: the dlogits an
    accumulate 1 call starts from (None: accumulate 0 into a NaN-filled tensor).  teacher "own": the case's; "alias": the logits tensor
    itself; "copy": a copy of it."""
    B, T, Cn = case["B"], case["T"], case["C"]
    x = _dev(case["logits"])
    u = _dev(case["teacher"]) if teacher == "own" else x if teacher == "alias" else x.clone()
    fl = None if case["frame_len"] is None else _dev(case["frame_len"])
    out = torch.full((B, T, Cn), float("nan"), device="cuda") if old is None else _dev(old)
    dlb = torch.full((B * T, 64), 0x7FC07FC0, dtype=torch.int32, device="cuda") if want_dlb else None
    got, klf, klc = kd.kd_grad(x, u, fl, case["inv_temp"], case["mode"], case["grad_scale"], out=out, accumulate=old is not None, dlb=dlb, return_kl=True)
    assert got is out
    torch.cuda.synchronize()
    return dict(dlogits=out.cpu().numpy(), dlb=None if dlb is None else dlb.cpu().numpy().view(np.uint32), kl_frame=klf.cpu().numpy(), kl_clip=klc.cpu().numpy())


@pytest.fixture(scope="module")
def runs():
    """every case once with accumulate 0 and once with accumulate 1 on old_rows: shared by the tests below, read-only"""
    out = {}
    for name, c in CASES.items():
        o = P.old_rows(c)
        out[name] = (_run(c), o, _run(c, old=o))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1
def test_every_case_lies_within_the_bound_of_the_fp64_reference(runs):
    worst_g = worst_a = worst_k = 0.0
    fails = []
    for name, c in CASES.items():
        r0, o, r1 = runs[name]
        g, a, k = P.compare_grad(c, r0["dlogits"]), P.compare_grad(c, r1["dlogits"], old=o), P.compare_kl(c, r0["kl_frame"])
        worst_g, worst_a, worst_k = max(worst_g, g), max(worst_a, a), max(worst_k, k)
        if not (g <= 1 and a <= 1 and k <= 1):
            fails.append((name, g, a, k))
    print(f"worst err / bound over {len(CASES)} cases: dlogits {worst_g:.4g} (accumulate {worst_a:.4g}) at K = {P.K}, kl_frame {worst_k:.4g} at K_KL = {P.K_KL}; "
          f"in units of K_HOST: {worst_g * 4:.4g}, of K_HOST_KL: {worst_k * 4:.4g}")
    assert len(runs) == len(P.cases()) == 90
    assert not fails, fails[:5]


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("how", ("alias", "copy"))
def test_a_teacher_equal_to_the_student_gives_zero_exactly(how):
    for name, c in CASES.items():
        r = _run(c, teacher=how)
        inside = P.inside_of(c)
        assert (r["dlogits"] == 0).all() and (r["kl_frame"] == 0).all() and (r["kl_clip"] == 0).all(), name
        assert not np.signbit(r["kl_frame"]).any() and not np.signbit(r["dlogits"][~inside]).any(), name
        o = P.old_rows(c)
        ra = _run(c, old=o, teacher=how)
        assert (ra["dlogits"] == o).all(), name
        assert np.array_equal(ra["dlb"], P.dlb_of(ra["dlogits"])), name


# ------------------------------------------------------------------------------------------------ 3, 4, 5, 7
def test_accumulate_is_one_fp32_addition_dlb_the_bf16_of_the_final_rows_kl_clip_the_ascending_sum(runs):
    saw_tail = 0
    for name, c in CASES.items():
        r0, o, r1 = runs[name]
        inside = P.inside_of(c)
        want = np.where(inside[..., None], (o + r0["dlogits"]).astype(np.float32), o)      # float32 + float32 in numpy: one rounding
        assert np.array_equal(_bits(r1["dlogits"]), _bits(want)), f"{name}: accumulate is not old + G in one fp32 addition (or a row past the end moved)"
        assert np.array_equal(r0["dlb"], P.dlb_of(r0["dlogits"])) and np.array_equal(r1["dlb"], P.dlb_of(r1["dlogits"])), f"{name}: dlb is not the bf16 of the final rows"
        assert np.array_equal(_bits(r0["kl_clip"]), _bits(P.clip_sum(r0["kl_frame"], c))), f"{name}: kl_clip is not the ascending sum of kl_frame"
        assert np.array_equal(_bits(r0["kl_frame"]), _bits(r1["kl_frame"])), name
        if c["fkind"] == "mix" and (~inside).any():                # both inputs hold NaN there (kd_parity.make_case)
            assert np.isnan(c["logits"][~inside]).all() and np.isnan(c["teacher"][~inside]).all()
            assert (_bits(r0["dlogits"][~inside]) == 0).all() and (_bits(r0["kl_frame"][~inside]) == 0).all(), f"{name}: a row past the end is not +0"
            assert np.array_equal(_bits(r1["dlogits"][~inside]), _bits(o[~inside])), f"{name}: accumulate touched a row past the end"
            assert np.isfinite(r0["dlogits"]).all() and np.isfinite(r0["kl_clip"]).all() and np.isfinite(r1["dlogits"]).all()
            saw_tail += 1
    assert saw_tail >= 10


# ------------------------------------------------------------------------------------------------ 6
def test_two_runs_are_bit_identical(runs):
    for name, c in CASES.items():
        r0, o, r1 = runs[name]
        again, again1 = _run(c), _run(c, old=o)
        for k in ("dlogits", "dlb", "kl_frame", "kl_clip"):
            assert np.array_equal(_bits(r0[k]), _bits(again[k])) and np.array_equal(_bits(r1[k]), _bits(again1[k])), (name, k)


# ------------------------------------------------------------------------------------------------ 8
def test_every_refusal_fires_before_a_launch(lib):
    from test_kd import check_kd_grad_refusals
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    check_kd_grad_refusals(lib)                              # pointers into nowhere: a launch would fault
    torch.cuda.synchronize()
    x = torch.zeros((2, 16, 8), device="cuda")
    for bad in (dict(inv_temp=0.0), dict(mode="max"), dict(out=torch.zeros((2, 16, 9), device="cuda")), dict(accumulate=True),
                dict(dlb=torch.zeros((32, 64), device="cuda")), dict(lengths=[1.5, 2.0])):
        with pytest.raises((ValueError, _lib.IsharaError)):
            kd.kd_grad(x, x, **bad)
    with pytest.raises(_lib.IsharaError, match="dlogits overlaps logits"):
        kd.kd_grad(x, x, out=x)
    with pytest.raises(_lib.IsharaError, match="GPU"):
        kd.kd_grad(x.cpu(), x)


# ------------------------------------------------------------------------------------------------ 9
def test_a_captured_graph_replays_the_call(lib):
    c = next(c for c in P.cases() if c["C"] == 60 and c["T"] == 33 and c["fkind"] != "none")
    B, T, Cn = c["B"], c["T"], c["C"]
    x, u, fl = _dev(np.nan_to_num(c["logits"])), _dev(np.nan_to_num(c["teacher"])), _dev(c["frame_len"])
    out, dlb = torch.zeros((B, T, Cn), device="cuda"), torch.zeros((B * T, 64), dtype=torch.int32, device="cuda")
    klf, klc = torch.zeros((B, T), device="cuda"), torch.zeros((B,), device="cuda")

    def run():
        _lib.check(lib.ishara_kd_grad(None, _lib.ptr(x), _lib.ptr(u), B, T, Cn, C.c_float(c["inv_temp"]), c["mode"], _lib.ptr(fl), C.c_float(c["grad_scale"]),
                                      _lib.ptr(out), 0, _lib.ptr(dlb), _lib.ptr(klf), _lib.ptr(klc), _lib.stream()), "ishara_kd_grad")
    run()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (out, dlb, klf, klc)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for t in (out, klf, klc):
        t.fill_(float("nan"))
    dlb.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for t, e in zip((out, dlb, klf, klc), eager):
        assert torch.equal(t.view(torch.int32), e.view(torch.int32))
    u.copy_(x)                                               # the graph follows its buffers: the teacher now equals the student
    graph.replay()
    torch.cuda.synchronize()
    assert (out == 0).all() and (klc == 0).all()


# ------------------------------------------------------------------------------------------------ 10
def _kd_oracle(kw, mode, W, x, y, rows, seed, lam, tau, ctc_w):
    """The step's gradients in float64 under autograd: ctc_w * CTC + lam * tau^2 * mean_b (sum_t or mean_t) KL.  Returns (grads of the
    sum, |CTC share|, |KD share|, the batch's mean KL), the shares being the L2 norms over all parameters of the two terms' own gradients."""
    import torch.nn.functional as F
    from oracle import ishara_oracle as O
    from test_model_gpu import _oracle_cfg
    ocfg = _oracle_cfg(kw, 0.0)
    Pm = O.to_torch(W, torch.float64)
    logits, _ = O.forward(Pm, torch.from_numpy(x).to(torch.float64), ocfg, training=True, seed=seed)
    ctc = ctc_w * O.ctc_loss(torch.from_numpy(y).long(), logits)
    kl = F.kl_div(F.log_softmax(logits / tau, -1), F.softmax(torch.from_numpy(rows).to(torch.float64) / tau, -1), reduction="none").sum(-1)      # [B, T]
    per_clip = kl.mean(1) if mode == 1 else kl.sum(1)
    kdl = lam * tau * tau * per_clip.mean()
    names = [k for k, v in Pm.items() if v.requires_grad]
    gc = torch.autograd.grad(ctc, [Pm[k] for k in names], retain_graph=True, allow_unused=True)
    gk = torch.autograd.grad(kdl, [Pm[k] for k in names], allow_unused=True)
    z = lambda g, k: torch.zeros_like(Pm[k]) if g is None else g
    grads = {k: (z(a, k) + z(b, k)).numpy() for k, a, b in zip(names, gc, gk)}
    norm = lambda gs: float(np.sqrt(sum(float((g ** 2).sum()) for g in gs if g is not None)))
    return grads, norm(gc), norm(gk), float(per_clip.mean().detach())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["tiny", "variant"])          # variant: B T = 256, the padded 16-bit dlb feeds the classifier's GEMMs
def test_the_whole_model_against_the_oracle(name, mode, dtype):
    from oracle import ishara_oracle as O
    from test_model_gpu import BF16_TOL, CFGS, _build, _oracle_cfg, _perturb
    kw = CFGS[name]
    B, T = kw["B"], kw["input_shape"][0]
    tau, ctc_w = 2.0, 0.5
    lam = 2.0 * (T if mode == 1 else 1)                      # the mean over frames divides by T: the same share of the gradient in both modes
    model = _build(kw, dtype, 0.0)
    W = _perturb(model)
    x, y = O.synthetic_batch(_oracle_cfg(kw, 0.0), B, seed=1)
    rows = (2.0 * np.random.default_rng(26).standard_normal((B, T, model.C))).astype(np.float32)
    for k, v in dict(kd_weight=lam, kd_temperature=tau, kd_ctc_weight=ctc_w, kd_normalise=mode == 1).items():
        setattr(model.optimizer, k, v)
    loss_t, logits_t = model.loss_and_gradients(x, y, seed=4242, teacher_logits=_dev(rows))
    torch.cuda.synchronize()
    grads = model.get_gradients()
    ref, share_ctc, share_kd, ref_kl = _kd_oracle(kw, mode, W, x, y, rows, 4242, lam, tau, ctc_w)
    print(f"{name} mode {mode} {dtype}: |grad CTC| {share_ctc:.4g}, |grad KD| {share_kd:.4g}")
    assert share_kd >= 0.5 * share_ctc, "the distillation term is too small a share of the reference gradient to be tested by it"
    bad, worst = [], 0.0
    gscale = max(float(np.abs(v).max()) for v in ref.values())
    for n, rg in ref.items():
        gg = grads[n]
        if np.abs(rg).max() < 1e-6 * gscale:                    # analytically zero (a conv bias in front of BatchNorm): test_model_gpu's rule
            if np.abs(gg).max() > (1e-3 if dtype == "f32" else 3e-2) * gscale: bad.append((n, float(np.abs(gg).max() / gscale)))
        elif dtype == "f32":
            e = float(np.abs(gg - rg).max() / np.abs(rg).max())
            worst = max(worst, e)
            if e > 1e-3: bad.append((n, e))                     # test_model_gpu._check_train_step's f32 tolerance (a literal there)
        else:
            e = float(np.linalg.norm(gg - rg) / np.linalg.norm(rg))
            worst = max(worst, e)
            if e > (BF16_TOL["grad_small"] if rg.size <= 8 else BF16_TOL["grad"]): bad.append((n, e))
    print(f"worst gradient error {worst:.4g}")
    assert not bad, f"gradient mismatch ({len(bad)}/{len(ref)}): {sorted(bad, key=lambda t: -t[1])[:8]}"
    st = model.kd_stats()
    # |d KL_t| <= max_c |d z| / tau * sum_c |ps - pt| <= 2 / tau * the logits' error, for which test_model_gpu's own tolerances stand
    lerr = 1e-4 if dtype == "f32" else BF16_TOL["logits"]
    assert st["clips"] == B and st["per_frame"] == (mode == 1)
    assert abs(st["kl"] - ref_kl) <= (1 if mode == 1 else T) * lerr * 2 / tau + 1e-5 * ref_kl, (st["kl"], ref_kl)
    # the loss returned stays the label's CTC loss, unweighted
    ref_loss = float(O.ctc_loss(torch.from_numpy(y).long(), torch.from_numpy(logits_t.cpu().numpy()).to(torch.float64)))
    assert abs(float(loss_t.item()) - ref_loss) <= 1e-5 * abs(ref_loss) + 1e-4


# ------------------------------------------------------------------------------------------------ 11
KW = dict(dim=128, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(64, 36), num_conv_per_block=0, squeeze_expansion=4, top_dim=128)


def _batch(B, T, F, L, Cn, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, T, F)).astype(np.float32)
    y = np.full((B, L), Cn - 1, np.int64)
    for b in range(B):
        n = int(g.integers(3, 12))
        y[b, :n] = g.integers(0, Cn - 1, n)
    return x, y


@pytest.mark.parametrize("dtype", ("bf16", "f32"))
@pytest.mark.parametrize("masked", (False, True))
def test_loss_backward_kd_with_the_students_own_logits_as_teacher_equals_the_entries_without_it(dtype, masked):
    B, s = 4, 0.75                                           # M = B T = 256: the padded-dlb classifier route
    m = get_model(dropout_rate=0.0, head_dropout=0.0, conformer_attn_dropout=0.0, dtype=dtype, max_batch=B, seed=3, **KW)
    T, Cn, L = m.T, m.C, m._cfg.max_label_len
    x, y = _batch(B, T, 36, L, Cn, 1)
    fl = torch.tensor([64, 40, 17, 64], dtype=torch.int32, device="cuda") if masked else None
    flkw = dict(frame_lengths=fl) if masked else {}
    yd = torch.from_numpy(y).cuda()
    klf, klc = torch.full((B, T), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")

    def forward():
        return m(x, training=True, seed=7, **flkw)

    # --- against ishara_loss_backward_ex
    logits = forward()
    _lib.check(m._lib.ishara_loss_backward_ex(m._h, _lib.ptr(logits), _lib.ptr(yd), B, _lib.ptr(m._loss_buf), _lib.ptr(m._nll_buf), C.c_float(s), _lib.ptr(fl),
                                              _lib.stream()), "ishara_loss_backward_ex")
    ref, ref_loss = m.grads.clone(), m._loss_buf.clone()
    logits = forward()
    stage = _lib.KdStage(logits.data_ptr(), 0.5, 1, 3.0, klf.data_ptr(), klc.data_ptr())
    _lib.check(m._lib.ishara_loss_backward_kd(m._h, _lib.ptr(logits), _lib.ptr(yd), B, _lib.ptr(m._loss_buf), _lib.ptr(m._nll_buf), C.c_float(s), _lib.ptr(fl),
                                              C.byref(stage), None, _lib.stream()), "ishara_loss_backward_kd")
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    assert torch.equal(m.grads, ref), f"{dtype}: max diff {(m.grads - ref).abs().max().item():.3g}"
    assert torch.equal(m._loss_buf, ref_loss) and (klf == 0).all() and (klc == 0).all()
    # both stages NULL: ishara_loss_backward_ex itself, bit for bit
    logits = forward()
    _lib.check(m._lib.ishara_loss_backward_kd(m._h, _lib.ptr(logits), _lib.ptr(yd), B, _lib.ptr(m._loss_buf), _lib.ptr(m._nll_buf), C.c_float(s), _lib.ptr(fl),
                                              None, None, _lib.stream()), "ishara_loss_backward_kd")
    assert torch.equal(m.grads.view(torch.int32), ref.view(torch.int32))
    # --- with the n-best stage, against ishara_loss_backward_nbest
    g = torch.Generator(device="cuda").manual_seed(3)
    N = 3
    hyp_idx = torch.randint(0, Cn - 1, (B, N, T), generator=g, device="cuda", dtype=torch.int32)
    hyp_len = torch.randint(1, 9, (B, N), generator=g, device="cuda", dtype=torch.int32)
    coef = torch.randn((B, N), generator=g, device="cuda") * 0.3
    ws = torch.empty(mwer.workspace_bytes(m._lib, B, T, N, L), dtype=torch.uint8, device="cuda")
    logits = forward()
    _lib.check(m._lib.ishara_loss_backward_nbest(m._h, _lib.ptr(logits), _lib.ptr(yd), B, _lib.ptr(m._loss_buf), _lib.ptr(m._nll_buf), C.c_float(s), _lib.ptr(fl),
                                                 _lib.ptr(hyp_idx), _lib.ptr(hyp_len), N, T, L, _lib.ptr(coef), C.c_float(0.4), _lib.ptr(ws), _lib.stream()),
               "ishara_loss_backward_nbest")
    ref_nb = m.grads.clone()
    assert not torch.equal(ref_nb, ref)
    nb = _lib.NbestStage(hyp_idx.data_ptr(), hyp_len.data_ptr(), N, T, L, coef.data_ptr(), 0.4, ws.data_ptr())
    for st in (stage, None):                                 # with the distillation stage on the student's own logits, and without it
        logits = forward()
        if st is not None:
            st.teacher = logits.data_ptr()
        _lib.check(m._lib.ishara_loss_backward_kd(m._h, _lib.ptr(logits), _lib.ptr(yd), B, _lib.ptr(m._loss_buf), _lib.ptr(m._nll_buf), C.c_float(s), _lib.ptr(fl),
                                                  None if st is None else C.byref(st), C.byref(nb), _lib.stream()), "ishara_loss_backward_kd")
        torch.cuda.synchronize()
        assert torch.equal(m.grads, ref_nb), f"{dtype}: max diff {(m.grads - ref_nb).abs().max().item():.3g}"
    assert torch.equal(m.grads.view(torch.int32), ref_nb.view(torch.int32))      # without the stage: bit for bit


# ------------------------------------------------------------------------------------------------ 12 - 14
TINY = dict(dim=32, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(48, 20), kernel_sizes=[5, 3], num_conv_per_block=2, num_heads=4,
            transformer_kernel_size=7)


def _tiny(seed=3, dim=32, **opt):
    m = get_model(dropout_rate=0.0, head_dropout=0.0, conformer_attn_dropout=0.0, dtype="f32", max_batch=3, seed=seed, **dict(TINY, dim=dim))
    m.optimizer.learning_rate = 4e-3
    for k, v in opt.items():
        setattr(m.optimizer, k, v)
    return m


@pytest.mark.parametrize("opt", (dict(), dict(accumulate_steps=2), dict(global_clipnorm=1.0, skip_nonfinite=True), dict(awp_delta=0.2), dict(mwer_nbest=4)),
                         ids=("plain", "accumulate", "clip", "awp", "mwer"))
def test_train_on_batch_with_a_teacher_gives_finite_gradients_and_runs_it_once_per_microbatch(opt):
    m = _tiny(kd_weight=1.0, **opt)
    big = _tiny(seed=5, dim=64)                              # a wider teacher of the same T, C and features
    calls = []

    def teacher(xd, fl):
        calls.append((tuple(xd.shape), fl))
        return big(xd, training=False)

    m.set_teacher(teacher)
    x, y = _batch(3, 48, 20, m._cfg.max_label_len, m.C, 2)
    before = m.params.clone()
    for step in range(2):
        loss = m.train_on_batch(x, y, seed=step)
    torch.cuda.synchronize()
    assert calls == [((3, 48, 20), None)] * 2, "the teacher runs once per train_on_batch call (AWP's second pass reuses its rows)"
    assert np.isfinite(float(loss)) and torch.isfinite(m.grads).all() and torch.isfinite(m.params).all()
    assert m.grads[:m.n_train].abs().max() > 0 and not torch.equal(m.params, before)
    st = m.kd_stats()
    assert np.isfinite(st["kl"]) and st["kl"] > 0 and st["clips"] == 3 and st["per_frame"]
    if "mwer_nbest" in opt:
        assert m.mwer_stats()["clips"] == 3
    assert m._kd_rows is None


def test_a_model_and_a_list_of_models_teach_like_their_rows_and_a_missing_teacher_is_refused(tmp_path):
    x, y = _batch(3, 48, 20, 64, 60, 2)
    t1, t2 = _tiny(seed=5, dim=64), _tiny(seed=6)
    from ishara_amd.ensemble import combine_logits
    rows1 = t1(x, training=False)
    fused = combine_logits([rows1, t2(x, training=False)], [1, 3], "linear")
    for teacher, kw, rows in ((t1, {}, rows1), ([t1, t2], dict(weights=[1, 3], mode="linear"), fused)):
        a, b = _tiny(kd_weight=0.5, kd_temperature=3.0), _tiny(kd_weight=0.5, kd_temperature=3.0)
        a.set_teacher(teacher, **kw)
        a.train_on_batch(x, y, seed=1)
        b.train_on_batch(x, y, seed=1, teacher_logits=rows)
        torch.cuda.synchronize()
        assert torch.equal(a.params.view(torch.int32), b.params.view(torch.int32)) and torch.equal(a.grads, b.grads)
    # the state holds the options, not the teacher: a restored run says so at its first step
    path = a.save_state(str(tmp_path / "run"))
    c = _tiny()
    c.load_state(path)
    assert c.optimizer.kd_options() == a.optimizer.kd_options() and c._teacher is None
    with pytest.raises(_lib.IsharaError, match="no teacher is attached"):
        c.train_on_batch(x, y, seed=2)
    with pytest.raises(ValueError, match="teacher_logits must be"):
        c.train_on_batch(x, y, seed=2, teacher_logits=rows1[:2])
    c.set_teacher([t1, t2], weights=[1, 3], mode="linear")
    c.train_on_batch(x, y, seed=2)
    a.train_on_batch(x, y, seed=2)
    torch.cuda.synchronize()
    assert torch.equal(a.params.view(torch.int32), c.params.view(torch.int32))


@pytest.mark.parametrize("normalise", (True, False))
def test_kd_stats_is_the_reference_on_the_downloaded_logits(normalise):
    tau = 2.0
    m = _tiny(kd_weight=1.0, kd_temperature=tau, kd_normalise=normalise)
    x, y = _batch(3, 48, 20, m._cfg.max_label_len, m.C, 3)
    rows = (2.0 * np.random.default_rng(27).standard_normal((3, 48, 60))).astype(np.float32)
    _, logits = m.loss_and_gradients(x, y, seed=1, teacher_logits=_dev(rows))
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    ref = kd.kd_reference(lg, rows, 1.0 / tau, "mean" if normalise else "sum")
    T = 48
    scale = 1.0 + (1.0 / tau) * (np.abs(lg).max(-1) + np.abs(rows).max(-1))
    klf = m._kd["kl_frame"][:3].cpu().numpy()
    assert (np.abs(klf - ref["kl_frame"]) <= P.K_KL * P.EPS * scale).all()
    # the clip's value: the frames' bounds, the T sequential additions (each within 2^-24 of the partial sum) and the final product
    w = ref["w"]
    bound = w * ((P.K_KL * P.EPS * scale).sum(1) + T * P.EPS * ref["kl_frame"].sum(1)) + P.EPS * ref["kl_clip"]
    klc = m._kd["kl_clip"][:3].cpu().numpy()
    assert (np.abs(klc - ref["kl_clip"]) <= bound).all(), (klc, ref["kl_clip"], bound)
    st = m.kd_stats()
    assert abs(st["kl"] - ref["kl_clip"].mean()) <= bound.mean() and st["per_frame"] == normalise and st["clips"] == 3


def test_the_option_off_leaves_a_step_bit_equal_and_allocates_nothing():
    a, b = _tiny(), _tiny(kd_weight=0.0, kd_temperature=4.0, kd_ctc_weight=0.3, kd_normalise=False)      # a: an optimizer built without the options
    calls = []
    b.set_teacher(lambda xd, fl: calls.append(1))
    x, y = _batch(3, 48, 20, a._cfg.max_label_len, a.C, 4)
    for step in range(2):
        a.train_on_batch(x, y, seed=step)
        b.train_on_batch(x, y, seed=step)
    torch.cuda.synchronize()
    assert torch.equal(a.params.view(torch.int32), b.params.view(torch.int32)) and b._kd is None and not calls
    rows = _dev((2.0 * np.random.default_rng(28).standard_normal((3, 48, 60))).astype(np.float32))
    c = _tiny(kd_weight=1.0, kd_start_step=2)                # not started during these two steps
    for step in range(2):
        c.train_on_batch(x, y, seed=step, teacher_logits=rows)
    assert torch.equal(a.params.view(torch.int32), c.params.view(torch.int32)) and c._kd is None
    c.train_on_batch(x, y, seed=2, teacher_logits=rows)
    a.train_on_batch(x, y, seed=2)
    assert c._kd is not None and not torch.equal(a.params, c.params)


# ------------------------------------------------------------------------------------------------ 15
@pytest.mark.parametrize("reduction", ("mean", "sum", "none"))
def test_kd_loss_backward_on_an_encoder_output_equals_kd_grad_by_hand(reduction):
    from ishara_amd import ConformerEncoder
    B, T, d, tau = 2, 16, 32, 2.0
    enc = ConformerEncoder(d, 1, 4, seq_len=T, max_batch=B, dtype="f32", seed=3)
    enc.train()
    g = torch.Generator().manual_seed(6)
    x = torch.randn((B, T, d), generator=g).cuda().requires_grad_(True)
    teacher = (torch.randn((B, T, d), generator=g) * 2).cuda()
    il = torch.tensor([16, 11])
    y = enc(x)
    y.retain_grad()
    loss = kd.kd_loss(y, teacher, il, temperature=tau, normalise=True, reduction=reduction)
    up = torch.tensor([0.5, -2.0], device="cuda")
    (loss * up).sum().backward() if reduction == "none" else loss.backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    yd = y.detach().contiguous()
    factor = 1.0 / B if reduction == "mean" else 1.0
    by_hand, klf, klc = kd.kd_grad(yd, teacher, il, 1.0 / tau, "mean", tau * factor, return_kl=True)
    if reduction == "none":
        by_hand = by_hand * up[:, None, None]
        assert torch.equal(loss.detach(), klc * (tau * tau))
    else:
        assert torch.allclose(loss.detach(), (klc * (tau * tau)).sum() * factor)
    assert torch.equal(y.grad, by_hand) and (by_hand[1, 11:] == 0).all()
    ref = kd.kd_reference(yd.cpu().numpy(), teacher.cpu().numpy(), 1.0 / tau, "mean", il.numpy())
    assert np.allclose(klc.cpu().numpy(), ref["kl_clip"], rtol=1e-4, atol=1e-6)
