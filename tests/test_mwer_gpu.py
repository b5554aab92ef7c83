"""GPU: ishara_ctc_nbest_grad (csrc/ctc_nbest_grad.hip), ishara_mwer_weights (csrc/mwer_weights.hip), ishara_loss_backward_nbest
(csrc/keras_hybrid.hip) and their Python surface over the cases of tests/mwer_parity.py.
  1  N = 1, coef = 1: dlogits and dlb bit-equal to ishara_op_ctc_loss (ishara_ctc_loss_ex with frame_len) on every slot of the seam cases
  2  every case within the per-term bound of the fp64 reference; status and logp equal to ishara_ctc_score_nbest's; rows past a clip's end
     +0; NaN past a clip's end never read
  3  accumulate = 1 on a random base equals base + G in torch fp32 bit for bit, dlb the bf16 of that sum; two runs bit-identical
  4  ishara_mwer_weights: dist / tlen exact, post within the vote bound, risk / coef bit-equal to the float32 recomputation from post
  5  plumbing, exact: ishara_loss_backward_nbest with hyp = labels, N = 1, coef = 1 at loss_scale = risk_scale = s / 2 gives the gradients
     of ishara_loss_backward at s bit for bit, in bf16 and in f32
  6  Python: train_on_batch with Optimizer(mwer_nbest=4) alone and with accumulation, clipping and AWP; mwer_stats against mwer_reference;
     mwer_nbest = 0 leaves a step bit-equal; mwer_loss(...).backward() on a ConformerEncoder output equals ctc_nbest_grad called by hand"""
import ctypes as C

import numpy as np
import pytest
import torch

import mwer_parity as P
import rescore_parity as RP
from ishara_amd import _lib, get_model, mwer, rescore

pytestmark = pytest.mark.gpu

GRAD = {c["name"]: c for c in P.grad_cases()}
WEIGHT = {c["name"]: c for c in P.weight_cases()}
SEAM_CASES = ("seams-64", "seams-272", "tight", "ragged", "T1", "T9", "C64-blank0")


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the cases' arrays are read-only


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _run(case, coef=None, grad_scale=None, hyp=None, out=None, accumulate=False, want_dlb=False, return_logp=True):
    idx, ln = hyp if hyp is not None else (case["hyp_idx"], case["hyp_len"])
    fl = None if case["frame_len"] is None else _dev(case["frame_len"])      # a device tensor is handed on unchecked: 0 reaches the kernel
    dlb = torch.full((case["B"] * case["T"], 64), 0x7FC07FC0, dtype=torch.int32, device="cuda") if want_dlb else None
    r = mwer.ctc_nbest_grad(_dev(case["logits"]), _dev(idx), _dev(ln), _dev(case["coef"] if coef is None else coef), fl,
                            case["grad_scale"] if grad_scale is None else grad_scale, out=out, accumulate=accumulate, max_len=case["max_len"],
                            return_logp=return_logp, blank=case["blank"], dlb=dlb)
    return r, dlb


def _bf16_rows(g):
    """[B, T, C] fp32 tensor -> the padded bf16 copy as int32 [B * T, 64] packed pairs (128 classes)"""
    B, T, Cn = g.shape
    pad = torch.zeros((B * T, 128), dtype=torch.float32, device=g.device)
    pad[:, :Cn] = g.reshape(B * T, Cn)
    return pad.to(torch.bfloat16).view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the loss kernel's bits
@pytest.mark.parametrize("name", SEAM_CASES)
def test_one_hypothesis_with_coef_one_is_the_loss_kernel_bit_for_bit(lib, name):
    case = GRAD[name]
    B, N, T, Cn, bl = case["B"], case["N"], case["T"], case["C"], case["blank"]
    x = _dev(case["logits"])
    fl = None if case["frame_len"] is None else _dev(case["frame_len"])
    checked = 0
    for n in range(N):
        y, ok = P.label_rows(case, n)
        if not ok.any():
            continue
        L = y.shape[1]
        one = np.ones((B, 1), np.float32)
        (G, _, st), dlb = _run(case, coef=one, grad_scale=0.375, hyp=(np.ascontiguousarray(case["hyp_idx"][:, n:n + 1]), np.ascontiguousarray(case["hyp_len"][:, n:n + 1])),
                               want_dlb=True)
        ws = torch.empty(int(lib.ishara_ctc_workspace_bytes(B, T, L)), dtype=torch.uint8, device="cuda")
        nll = torch.empty(B, dtype=torch.float32, device="cuda")
        ref = torch.empty((B, T, Cn), dtype=torch.float32, device="cuda")
        if fl is None:
            rdlb = torch.zeros((B * T, 64), dtype=torch.int32, device="cuda")
            _lib.check(lib.ishara_op_ctc_loss(_lib.ptr(x), _lib.ptr(_dev(y)), B, T, Cn, L, bl, _lib.ptr(nll), _lib.ptr(ref), C.c_float(0.375), _lib.ptr(ws),
                                              _lib.ptr(rdlb), _lib.stream()), "ishara_op_ctc_loss")
        else:                                                # the frame_len leg has no dlb: the bf16 of the rows stands in
            _lib.check(lib.ishara_ctc_loss_ex(_lib.ptr(x), _lib.ptr(_dev(y)), B, T, Cn, L, bl, _lib.ptr(nll), _lib.ptr(ref), C.c_float(0.375), _lib.ptr(ws),
                                              _lib.ptr(fl), None, 0, _lib.stream()), "ishara_ctc_loss_ex")
            rdlb = _bf16_rows(ref)
        torch.cuda.synchronize()
        ok = ok & (st.cpu().numpy()[:, 0] == 0)
        for b in np.nonzero(ok)[0]:
            assert np.array_equal(_bits(G[b].cpu().numpy()), _bits(ref[b].cpu().numpy())), f"{name}: slot {n} of clip {b}: dlogits differ from the loss kernel's"
            assert torch.equal(dlb[b * T:(b + 1) * T], rdlb[b * T:(b + 1) * T]), f"{name}: slot {n} of clip {b}: dlb differs"
            checked += 1
    assert checked >= 1


# ------------------------------------------------------------------------------------------------ 2. the fp64 reference
@pytest.mark.parametrize("name", sorted(GRAD))
def test_every_case_within_the_bound_of_the_fp64_reference(name):
    case = GRAD[name]
    (G, logp, st), _ = _run(case)
    fails, ratio = P.check_grad(case, G.cpu().numpy())
    print(f"{name}: gradient err / bound {ratio:.4g}")
    assert not fails, fails[:3]
    want = P.expected_status(case)
    assert np.array_equal(st.cpu().numpy(), want), st.cpu().tolist()
    fl = None if case["frame_len"] is None else _dev(case["frame_len"])
    slp, sst = rescore.ctc_score_nbest(_dev(case["logits"]), _dev(case["hyp_idx"]), _dev(case["hyp_len"]), fl, case["blank"], return_status=True)
    same = case["hyp_len"] <= case["max_len"]                # a slot longer than max_len is this kernel's own refusal
    assert np.array_equal(_bits(logp.cpu().numpy())[same], _bits(slp.cpu().numpy())[same]) and np.array_equal(st.cpu().numpy()[same], sst.cpu().numpy()[same])
    assert np.isneginf(logp.cpu().numpy()[~same]).all()


def test_a_skipped_slot_is_not_read_and_bad_slots_leave_their_neighbours_alone():
    case = GRAD["bad-slots"]
    want = P.expected_status(case)
    G, _ = _run(case, return_logp=False)
    idx = case["hyp_idx"].copy()
    coef = case["coef"].copy()
    idx[want != 0] = RP.DEAD_SYMBOL                          # the rows of the slots that take no part, overwritten
    ln = np.where(want != 0, -1, case["hyp_len"]).astype(np.int32)
    G2, _ = _run(case, hyp=(idx, ln), return_logp=False)
    assert torch.equal(G.view(torch.int32), G2.view(torch.int32)), "a slot that takes no part changed the gradient"
    coef[0, 0] = 0.0
    idx[0, 0] = RP.DEAD_SYMBOL
    ln0 = ln.copy()
    ln0[0, 0] = 3                                            # a live slot with coef 0 and a poisoned row: skipped, not read
    G3, _ = _run(case, coef=coef, hyp=(idx, ln0), return_logp=False)
    ln0[0, 0] = -1
    G4, _ = _run(case, coef=coef, hyp=(idx, ln0), return_logp=False)
    assert torch.equal(G3.view(torch.int32), G4.view(torch.int32)) and torch.isfinite(G3).all()


# ------------------------------------------------------------------------------------------------ 3. accumulate, dlb, determinism
@pytest.mark.parametrize("name", ("seams-64", "ragged", "N64", "C60-blank59", "seams-272"))
def test_accumulate_adds_by_one_fp32_addition_and_dlb_is_the_bf16_of_the_sum(name):
    case = GRAD[name]
    (G, _, _), dlb0 = _run(case, want_dlb=True)
    (Gb, _, _), _ = _run(case)
    assert torch.equal(G.view(torch.int32), Gb.view(torch.int32)), "two runs differ"
    assert torch.equal(dlb0, _bf16_rows(G))
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.randn(G.shape, device="cuda", generator=g) * 0.01
    want = base.clone()
    for b in range(case["B"]):
        tb = RP.clip_frames(case, b)
        want[b, :tb] = base[b, :tb] + G[b, :tb]              # rows past the clip's end stay as they are
    out = base.clone()
    (_, _, _), dlb = _run(case, out=out, accumulate=True, want_dlb=True)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "accumulate is not base + G in one fp32 addition"
    assert torch.equal(dlb, _bf16_rows(want)), "dlb is not the bf16 copy of the final rows"


# ------------------------------------------------------------------------------------------------ 4. the weights
@pytest.mark.parametrize("name", sorted(WEIGHT))
def test_weights_distances_exact_posterior_in_bound_risk_and_coef_recomputed(name):
    case = WEIGHT[name]
    it = None if case["inv_temp"] is None else torch.full((1,), float(case["inv_temp"]), dtype=torch.float32, device="cuda")
    got = mwer.mwer_weights(_dev(case["hyp_idx"]), _dev(case["hyp_len"]), _dev(case["logp"]), _dev(case["targets"]), 1.0 if it is None else it,
                            case["mode"] == 1, None if case["status"] is None else _dev(case["status"]))
    got = {k: v.cpu().numpy() for k, v in got.items()}
    fails, ratio = P.check_weights(case, got)
    print(f"{name}: posterior err / bound {ratio:.4g}")
    assert not fails, fails[:3]
    if name.startswith("dead-slots"):
        assert np.isnan(got["risk"][1]) and (got["dist"][1] == -1).all() and (got["coef"][1].view(np.uint32) == 0).all()


# ------------------------------------------------------------------------------------------------ 5. the model's second loss term
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
def test_loss_backward_nbest_on_the_label_halves_sum_to_the_plain_backward_bit_for_bit(dtype):
    B, s = 4, 1.0                                            # M = B T = 256: the padded-dlb classifier route; halves of a power-of-two product are exact
    m = get_model(dropout_rate=0.0, head_dropout=0.0, conformer_attn_dropout=0.0, dtype=dtype, max_batch=B, seed=3, **KW)
    T, Cn, L = m.T, m.C, m._cfg.max_label_len
    assert B * T >= 256 and (B * T) % 64 == 0
    x, y = _batch(B, KW["input_shape"][0], 36, L, Cn, 1)
    loss, logits = m.loss_and_gradients(x, y, seed=7, loss_scale=s)
    ref, ref_loss, ref_nll = m.grads.clone(), loss.clone(), m._nll_buf[:B].clone()
    yd = torch.from_numpy(y).cuda()
    hyp_idx = torch.where(yd == Cn - 1, torch.full_like(yd, -1), yd).to(torch.int32).reshape(B, 1, L).contiguous()
    hyp_len = (yd != Cn - 1).sum(1).to(torch.int32).reshape(B, 1).contiguous()
    coef = torch.ones((B, 1), dtype=torch.float32, device="cuda")
    ws = torch.empty(mwer.workspace_bytes(m._lib, B, T, 1, L), dtype=torch.uint8, device="cuda")
    logits2 = m(x, training=True, seed=7)
    assert torch.equal(logits2, logits)
    m._loss_buf.zero_()
    _lib.check(m._lib.ishara_loss_backward_nbest(m._h, _lib.ptr(logits2), _lib.ptr(yd), B, _lib.ptr(m._loss_buf), _lib.ptr(m._nll_buf), C.c_float(s / 2), None,
                                                 _lib.ptr(hyp_idx), _lib.ptr(hyp_len), 1, L, L, _lib.ptr(coef), C.c_float(s / 2), _lib.ptr(ws), _lib.stream()),
               "ishara_loss_backward_nbest")
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    assert torch.equal(m.grads.view(torch.int32), ref.view(torch.int32)), f"{dtype}: max diff {(m.grads - ref).abs().max().item():.3g}"
    assert torch.equal(m._loss_buf, ref_loss) and torch.equal(m._nll_buf[:B], ref_nll)      # loss and nll keep their meaning


# ------------------------------------------------------------------------------------------------ 6. Python
TINY = dict(dim=32, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(48, 20), kernel_sizes=[5, 3], num_conv_per_block=2, num_heads=4,
            transformer_kernel_size=7)


def _tiny(**opt):
    m = get_model(dropout_rate=0.0, head_dropout=0.0, conformer_attn_dropout=0.0, dtype="f32", max_batch=3, seed=3, **TINY)
    m.optimizer.learning_rate = 4e-3
    for k, v in opt.items():
        setattr(m.optimizer, k, v)
    return m


@pytest.mark.parametrize("opt", (dict(), dict(accumulate_steps=2), dict(global_clipnorm=1.0, skip_nonfinite=True), dict(awp_delta=0.2)),
                         ids=("plain", "accumulate", "clip", "awp"))
def test_train_on_batch_with_the_risk_term_gives_finite_gradients(opt):
    m = _tiny(mwer_nbest=4, **opt)
    x, y = _batch(3, TINY["input_shape"][0], 20, m._cfg.max_label_len, m.C, 2)
    before = m.params.clone()
    for step in range(2):
        loss = m.train_on_batch(x, y, seed=step)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and torch.isfinite(m.grads).all() and torch.isfinite(m.params).all()
    assert m.grads[:m.n_train].abs().max() > 0 and not torch.equal(m.params, before)
    st = m.mwer_stats()
    assert np.isfinite(st["risk"]) and st["risk"] >= 0 and 1 <= st["live_slots"] <= 12 and st["clips"] == 3


def test_mwer_stats_is_the_reference_risk_on_the_downloaded_logits():
    m = _tiny(mwer_nbest=4, mwer_temperature=2.0)
    x, y = _batch(3, TINY["input_shape"][0], 20, m._cfg.max_label_len, m.C, 3)
    _, logits = m.loss_and_gradients(x, y, seed=1)
    torch.cuda.synchronize()
    st, w = m.mwer_stats(), m._mwer
    lg, idx, ln = logits.cpu().numpy(), w["idx"][:3].cpu().numpy(), w["len"][:3].cpu().numpy()
    risks = []
    for b in range(3):
        hyps = [idx[b, n, :ln[b, n]].tolist() if ln[b, n] >= 0 else None for n in range(4)]
        tgt = [int(v) for v in y[b] if v != m.C - 1]
        ref = mwer.mwer_reference(lg[b], hyps, tgt, m.C - 1, 0.5, True)
        risks.append(ref["risk"])
        # the posterior moves by |d logp| * inv_temp at most per slot, the loss kernel's nll bound on each logp
        tol = 2 * 0.5 * max(P.NLL_ATOL + P.NLL_RTOL * abs(v) for v in ref["logp"] if np.isfinite(v)) * max(abs(ref["dist"]).max() / max(len(tgt), 1), 1.0)
        assert abs(float(w["risk"][b]) - ref["risk"]) <= tol + 1e-6, (b, float(w["risk"][b]), ref["risk"])
        assert np.array_equal(w["dist"][b].cpu().numpy(), ref["dist"])
    assert abs(st["risk"] - np.mean(risks)) <= 1e-3 and st["clips"] == 3


def test_the_option_off_leaves_a_step_bit_equal_and_allocates_nothing():
    a, b = _tiny(), _tiny(mwer_nbest=0, mwer_beam_width=16, mwer_weight=3.0)
    x, y = _batch(3, TINY["input_shape"][0], 20, a._cfg.max_label_len, a.C, 4)
    for step in range(2):
        a.train_on_batch(x, y, seed=step)
        b.train_on_batch(x, y, seed=step)
    torch.cuda.synchronize()
    assert torch.equal(a.params.view(torch.int32), b.params.view(torch.int32)) and b._mwer is None
    c = _tiny(mwer_nbest=4, mwer_start_step=2)               # not started during these two steps
    for step in range(2):
        c.train_on_batch(x, y, seed=step)
    assert torch.equal(a.params.view(torch.int32), c.params.view(torch.int32)) and c._mwer is None
    c.train_on_batch(x, y, seed=2)
    a.train_on_batch(x, y, seed=2)
    assert c._mwer is not None and not torch.equal(a.params, c.params)


def test_mwer_loss_backward_on_an_encoder_output_equals_ctc_nbest_grad_by_hand():
    from ishara_amd import ConformerEncoder
    from ishara_amd.ctc import pack_targets
    B, T, d = 2, 16, 32
    enc = ConformerEncoder(d, 1, 4, seq_len=T, max_batch=B, dtype="f32", seed=3)
    enc.train()
    g = torch.Generator().manual_seed(6)
    x = torch.randn((B, T, d), generator=g).cuda().requires_grad_(True)
    targets = torch.tensor([[3, 7, 7, 1], [5, 2, 0, 0]])
    tl, il = torch.tensor([4, 2]), torch.tensor([16, 11])
    y = enc(x)
    y.retain_grad()
    loss = mwer.mwer_loss(y, il, targets, tl, beam_width=8, nbest=4, temperature=1.5, blank=d - 1)
    loss.backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    yd = y.detach().contiguous()
    fl = il.to("cuda", torch.int32)
    t59 = pack_targets(targets, tl, 59, "cuda").to(torch.int32).contiguous()
    risk, grad, det = mwer.nbest_pipeline(yd, fl, t59, 8, 4, 1.5, True, d - 1, mwer.mwer_max_len(4), 1.0 / B)
    by_hand = mwer.ctc_nbest_grad(yd, det["hyp_idx"], det["hyp_len"], det["coef"], fl, 1.0 / B, max_len=mwer.mwer_max_len(4), blank=d - 1)
    assert torch.equal(y.grad.view(torch.int32), by_hand.view(torch.int32)) and torch.equal(grad, by_hand)
    assert torch.allclose(loss.detach(), risk.sum() / B) and (by_hand[1, 11:] == 0).all()
