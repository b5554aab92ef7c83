"""GPU: the Squeezeformer family's relative-position attention with per-clip lengths (csrc/relattn_len.hip) through the ishara_relattn_len_* pair,
and SqueezeformerEncoder / Squeezeformer with mask_padding=True (ishara_encoder_forward_lengths / _backward_lengths).

Operator level (cases, references and bounds of tests/relattn_len_parity.py; tests/test_relattn_len_mutants.py shows the bounds reject ordinary
mistakes): every case against fp64 in f32 and bf16, dropout 0 and 0.2; ishara_op_relattn_* (a NULL key_len) bit-equal to full lengths through the lane route; the
K / V rows at keys >= n[b] redrawn change no bit of o, lse, dq and the valid dk / dv rows, and the dk / dv rows past n[b] are exact zeros; a dead
clip is zeros.
Encoder level: both encoder cases against the masked fp64 restatement, full lengths against the plain call, a NULL input_len bit-equal to the
plain call, one Squeezeformer + ishara_amd.ctc_loss step with lengths, the mismatched backward refused."""
import ctypes as C

import numpy as np
import pytest
import torch

import r4_parity as R
import relattn_len_parity as L
from ishara_amd import _lib
from test_model_gpu import _log_observed
from test_ops_r4_gpu import DT, dev, host, run_relattn
from test_relattn_len_mutants import ENC_BOUND, encoder_errors

pytestmark = pytest.mark.gpu
BIT = ("o", "lse", "dq", "dk", "dv")      # deterministic outputs (du / dvb / dposp are fp32 atomics: order-dependent in the last bits)


def run_len(lib, case, n, dtype, seed, rate, route=0, redraw=False):
    B, H, T, dh = case
    d, Rr = H * dh, 2 * T - 1
    code, tdt = DT[dtype]
    inp = dict(R.relattn_inputs(case, dtype))
    if redraw:      # other finite values in the K and V rows the lengths mask
        g = np.random.default_rng(99)
        k2, v2 = np.array(inp["k"], copy=True), np.array(inp["v"], copy=True)
        for b, nb in enumerate(n):
            nb = min(max(nb, 0), T)
            k2[b, nb:] = L.MP.round_to(3 * g.standard_normal((T - nb, d)), dtype)
            v2[b, nb:] = L.MP.round_to(3 * g.standard_normal((T - nb, d)), dtype)
        inp["k"], inp["v"] = k2, v2
    q, k, v, dO = (dev(inp[x], tdt) for x in ("q", "k", "v", "dO"))
    pe, Wpos, u, vb = (dev(inp[x]) for x in ("pe", "Wpos", "u", "vb"))
    kl = torch.tensor(list(n), dtype=torch.int32, device="cuda")
    o, dq, dk, dv = (torch.full((B * T, d), float("nan"), dtype=tdt, device="cuda") for _ in range(4))
    lse = torch.full((B * H * T,), float("nan"), device="cuda")
    du, dvb = (torch.full((d,), float("nan"), device="cuda") for _ in range(2))
    dWpos = torch.full((d, d), float("nan"), device="cuda")
    dposp = torch.full((Rr, d), float("nan"), device="cuda")
    nbytes = int(lib.ishara_relattn_len_scratch_bytes(B, H, T, dh))
    assert nbytes > 0
    keep, sc = _lib.aligned(nbytes, "cuda")
    P = _lib.ptr
    _lib.check(lib.ishara_relattn_len_fwd(code, P(q), P(k), P(v), P(pe), P(Wpos), P(u), P(vb), P(o), P(lse), B, H, T, dh, seed, R.SITE, C.c_float(rate),
                                          P(kl), route, sc, _lib.stream()), "ishara_relattn_len_fwd")
    _lib.check(lib.ishara_relattn_len_bwd(code, P(q), P(k), P(v), P(u), P(vb), P(o), P(dO), P(dq), P(dk), P(dv), P(du), P(dvb), P(dWpos), P(dposp),
                                          B, H, T, dh, seed, R.SITE, C.c_float(rate), P(kl), route, sc, _lib.stream()), "ishara_relattn_len_bwd")
    torch.cuda.synchronize()
    del keep
    r3 = lambda t: host(t).reshape(B, T, d)
    return dict(o=r3(o), lse=host(lse).reshape(B, H, T), dq=r3(dq), dk=r3(dk), dv=r3(dv), du=host(du), dvb=host(dvb), dposp=host(dposp), dWpos=host(dWpos))


def _seed(case, rate):
    return R.dropout_seed(case, rate) if rate > 0 else 4242


@pytest.mark.parametrize("rate", L.RATES, ids=lambda r: f"drop{r}")
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", L.OP_CASES, ids=L.case_id)
def test_attention_with_lengths_matches_fp64(lib, case, dtype, rate):
    shape, n = case
    B, H, T, dh = shape
    seed = _seed(shape, rate)
    fwd = lib.ishara_debug_relattn_kernel_name(DT[dtype][0], 0, T, dh, 1).decode()
    mfma = fwd == "relattn_len_fwd_mfma_kernel"
    assert mfma == (dtype == "bf16" and dh in (32, 64)) and fwd.startswith("relattn_len_")
    fails = []
    for route in ((0, 1) if mfma else (0,)):      # both routes where both exist: the plan's choice, then the lane kernels forced
        got = run_len(lib, shape, n, dtype, seed, rate, route=route)
        for b in L.dead_clips(shape, n):      # zeros, the sentinel, and no trace in the gradients
            assert (got["lse"][b] == L.DEAD_LSE).all()
            assert not got["o"][b].any() and not got["dq"][b].any() and not got["dk"][b].any() and not got["dv"][b].any()
        for b, nb in enumerate(n):
            assert not got["dk"][b, min(nb, T):].any() and not got["dv"][b, min(nb, T):].any()
        is_mfma = mfma and route == 0
        obs, bad = L.compare(got, L.reference(shape, n, dtype, seed, rate), L.op_bounds(shape, n, dtype, seed, rate, mfma=is_mfma), shape, n)
        _log_observed(dict(test="relattn_len", case=L.case_id(case), dtype=dtype, rate=rate, route="mfma" if is_mfma else "lane", **obs))
        print(f"observed {'mfma' if is_mfma else 'lane'} {obs}")
        fails += bad
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rate", L.RATES, ids=lambda r: f"drop{r}")
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 2, 65, 64), (3, 4, 97, 32), (1, 2, 33, 8)], ids=lambda c: "B%d-H%d-T%d-dh%d" % c)
def test_a_null_key_len_is_full_lengths_through_the_lane_route_bit_for_bit(lib, shape, dtype, rate):
    """ishara_op_relattn_* (key_len NULL: every key) against key_len = T and key_len = T + 7 (clamped) with route 1: the same lane kernels, the same
    bits; and against fp64"""
    seed = _seed(shape, rate)
    want = run_relattn(lib, shape, dtype, seed, rate)
    got = run_len(lib, shape, (shape[2],) * shape[0], dtype, seed, rate, route=1)
    for name in BIT:
        assert np.array_equal(got[name], want[name]), name
    over = run_len(lib, shape, (shape[2] + 7,) * shape[0], dtype, seed, rate, route=1)      # clamped to T
    for name in BIT:
        assert np.array_equal(over[name], want[name]), name
    _, bad = R.compare(got, R.relattn_reference(shape, dtype, seed, rate), R.bounds(dtype), shape[0] * shape[2])
    assert not bad, "\n".join(bad)
    if lib.ishara_debug_relattn_kernel_name(DT[dtype][0], 0, shape[2], shape[3], 1) == b"relattn_len_fwd_mfma_kernel":
        # the plan's route has the MFMA forward here: full lengths against the UNMASKED fp64 reference, within that route's bounds
        full = (shape[2],) * shape[0]
        plan = run_len(lib, shape, full, dtype, seed, rate, route=0)
        assert not np.array_equal(plan["o"], want["o"])      # (another kernel ran)
        obs, bad = R.compare(plan, R.relattn_reference(shape, dtype, seed, rate), L.op_bounds(shape, full, dtype, seed, rate, mfma=True), shape[0] * shape[2])
        print(f"observed mfma {obs}")
        assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [L.OP_CASES[2], L.OP_CASES[3], L.OP_CASES[4], L.OP_CASES[6]], ids=L.case_id)
def test_the_masked_rows_of_k_and_v_are_never_read_into_a_result(lib, case, dtype):
    shape, n = case
    seed = _seed(shape, R.RATE)
    a = run_len(lib, shape, n, dtype, seed, R.RATE)
    b = run_len(lib, shape, n, dtype, seed, R.RATE, redraw=True)
    for name in BIT:
        assert np.array_equal(a[name], b[name]), name
    for bb, nb in enumerate(n):
        assert not b["dk"][bb, nb:].any() and not b["dv"][bb, nb:].any()
    for name in ("du", "dvb", "dposp", "dWpos"):      # atomics: equal up to the summation order
        assert np.allclose(a[name], b[name], rtol=1e-4, atol=1e-5 * float(np.abs(a[name]).max())), name


# ------------------------------------------------------------------ encoder level
def _encoder(name, dtype):
    from ishara_amd.squeezeformer import SqueezeformerEncoder
    cfg, T0, lens = L.ENC_CASES[name]
    x, Gm, P, y, dx = L.encoder_reference(name)
    enc = SqueezeformerEncoder(cfg["input_dim"], cfg["encoder_dim"], cfg["num_layers"], cfg["reduce_layer_index"], cfg["recover_layer_index"],
                               cfg["num_attention_heads"], cfg["feed_forward_expansion_factor"], 2, 0.0, 0.0, 0.0, 0.0, cfg["conv_kernel_size"],
                               cfg["half_step_residual"], seq_len=T0, max_batch=len(lens), dtype=dtype)
    enc.load_state_dict({k: v.detach().float() for k, v in P.items()})
    return enc


def _train_pass(enc, x, Gm, lens, mask_padding=True):
    xg = x.cuda().requires_grad_(True)
    if lens is None:
        y = enc.train()(xg)
    else:
        y, out_len = enc.train()(xg, lens, mask_padding=mask_padding)
        assert out_len.tolist() == enc.output_lengths(torch.as_tensor(lens)).tolist()
    (y * Gm.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu().double().numpy(), xg.grad.cpu().double().numpy(), {k: v.double().numpy() for k, v in enc.grad_state_dict().items()}


def _check_encoder(e, dtype, grads, ref_grads, name):
    print(f"observed {e}")
    bound = dict(ENC_BOUND[dtype], y=L.encoder_y_bound(name)) if dtype == "bf16" else ENC_BOUND[dtype]
    bad = [f"{q} {e[q]:.3e} > {b:.3e}" for q, b in bound.items() if not e[q] <= b]
    gscale = max(float(np.abs(v).max()) for v in ref_grads.values())
    for k, want in ref_grads.items():
        if np.abs(want).max() < 1e-6 * gscale and np.abs(grads[k]).max() > (1e-3 if dtype == "f32" else 3e-2) * gscale:
            bad.append(f"{k}: analytically zero, {np.abs(grads[k]).max():.3e}")
        elif dtype == "bf16" and want.size <= 16 and np.abs(want).max() >= 1e-6 * gscale:
            r = float(np.linalg.norm(grads[k] - want) / np.linalg.norm(want))
            if r > 0.25: bad.append(f"{k}: rel-L2 {r:.3e} > 0.25")
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(L.ENC_CASES))
def test_encoder_with_mask_padding_matches_the_masked_restatement(name, dtype):
    """output, dx and every parameter gradient; f32 at the tolerances of test_squeezeformer_other_shapes_vs_oracle, bf16 at those of
    test_squeezeformer_training_pass_matches_reference_autograd"""
    cfg, T0, lens = L.ENC_CASES[name]
    x, Gm, P, yo, dxo = L.encoder_reference(name)
    ref_grads = {k: v.grad.numpy() for k, v in P.items() if v.grad is not None}
    enc = _encoder(name, dtype)
    y, dx, grads = _train_pass(enc, x, Gm, torch.tensor(lens, dtype=torch.int32, device="cuda"))
    assert set(ref_grads) <= set(grads) and all(not grads[k].any() for k in set(grads) - set(ref_grads))      # (a layer the configuration never runs: zeros)
    e = encoder_errors(y, dx, grads, yo.numpy(), dxo.numpy(), ref_grads)
    _log_observed(dict(test="relattn_len_encoder", case=name, dtype=dtype, **e))
    _check_encoder(e, dtype, grads, ref_grads, name)
    # eval mode works too and needs no saved activations; the lengths may be a list
    with torch.no_grad():
        ye, _ = enc.eval()(x, list(lens), mask_padding=True)
        yp, _ = enc(x, list(lens))
    assert torch.isfinite(ye).all() and float((ye - yp).abs().max()) > 1e-3


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(L.ENC_CASES))
def test_full_lengths_give_the_plain_call(name, dtype):
    cfg, T0, lens = L.ENC_CASES[name]
    x, Gm, P, _, _ = L.encoder_reference(name)
    enc = _encoder(name, dtype)
    y0, dx0, g0 = _train_pass(enc, x, Gm, None)
    y1, dx1, g1 = _train_pass(enc, x, Gm, torch.full((len(lens),), T0, dtype=torch.int64))
    # the gradients fp64 knows to be zero (key_proj.bias: a constant added to every score of a row) are rounding noise in both passes: the fp64
    # reference names them, and they are held to the zero rule instead of being compared with each other
    _, _, P64, _, _ = L.encoder_reference(name, with_lengths=False)
    ref64 = {k: v.grad.numpy() for k, v in P64.items() if v.grad is not None}
    gscale = max(float(np.abs(v).max()) for v in ref64.values())
    zero = {k for k, v in ref64.items() if np.abs(v).max() < 1e-6 * gscale}
    assert zero and all(np.abs(g1[k]).max() <= (1e-3 if dtype == "f32" else 3e-2) * gscale for k in zero)
    keep = [k for k in ref64 if k not in zero]
    e = encoder_errors(y1, dx1, {k: g1[k] for k in keep}, y0, dx0, {k: g0[k] for k in keep})
    _check_encoder(e, dtype, g1, {k: g0[k] for k in keep}, name)


def test_a_null_input_len_is_the_plain_call_bit_for_bit():
    name = "dh32_no_recover"
    cfg, T0, lens = L.ENC_CASES[name]
    x, Gm, _, _, _ = L.encoder_reference(name)
    enc = _encoder(name, "bf16")
    lib, B = enc._lib, len(lens)
    xd, gd = x.cuda().contiguous(), Gm.cuda().contiguous()
    outs = []
    for lengths_entry in (False, True):
        y, dx = torch.empty(B, enc.T_out, enc.dim, device="cuda"), torch.empty(B, T0, cfg["input_dim"], device="cuda")
        if lengths_entry:
            _lib.check(lib.ishara_encoder_forward_lengths(enc._h, _lib.ptr(xd), B, _lib.ptr(y), 1, C.c_uint32(77), None, _lib.stream()), "forward_lengths")
            _lib.check(lib.ishara_encoder_backward_lengths(enc._h, _lib.ptr(gd), B, _lib.ptr(dx), None, _lib.stream()), "backward_lengths")
        else:
            _lib.check(lib.ishara_encoder_forward(enc._h, _lib.ptr(xd), B, _lib.ptr(y), 1, C.c_uint32(77), _lib.stream()), "forward")
            _lib.check(lib.ishara_encoder_backward(enc._h, _lib.ptr(gd), B, _lib.ptr(dx), _lib.stream()), "backward")
        torch.cuda.synchronize()
        outs.append((y.cpu(), dx.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_a_backward_that_disagrees_about_lengths_is_refused_and_a_modified_array_too():
    name = "dh32_no_recover"
    cfg, T0, lens = L.ENC_CASES[name]
    x, Gm, _, _, _ = L.encoder_reference(name)
    enc = _encoder(name, "f32")
    lib, B = enc._lib, len(lens)
    xd, gd = x.cuda().contiguous(), Gm.cuda().contiguous()
    kl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    y, dx = torch.empty(B, enc.T_out, enc.dim, device="cuda"), torch.empty(B, T0, cfg["input_dim"], device="cuda")
    _lib.check(lib.ishara_encoder_forward_lengths(enc._h, _lib.ptr(xd), B, _lib.ptr(y), 1, C.c_uint32(5), _lib.ptr(kl), _lib.stream()), "forward_lengths")
    for call, fn in ((lambda: lib.ishara_encoder_backward_lengths(enc._h, _lib.ptr(gd), B, _lib.ptr(dx), None, _lib.stream()), "ishara_encoder_backward_lengths"),
                     (lambda: lib.ishara_encoder_backward(enc._h, _lib.ptr(gd), B, _lib.ptr(dx), _lib.stream()), "ishara_encoder_backward")):
        rc = call()
        msg = lib.ishara_last_error().decode()
        assert rc != 0 and msg.startswith(fn + ":") and "was given" in msg and "not given" in msg, msg
    _lib.check(lib.ishara_encoder_backward_lengths(enc._h, _lib.ptr(gd), B, _lib.ptr(dx), _lib.ptr(kl), _lib.stream()), "backward_lengths")
    _lib.check(lib.ishara_encoder_forward(enc._h, _lib.ptr(xd), B, _lib.ptr(y), 1, C.c_uint32(5), _lib.stream()), "forward")
    assert lib.ishara_encoder_backward_lengths(enc._h, _lib.ptr(gd), B, _lib.ptr(dx), _lib.ptr(kl), _lib.stream()) != 0
    torch.cuda.synchronize()
    # autograd: the lengths array modified in place between forward and backward
    xg = x.cuda().requires_grad_(True)
    yy, _ = enc.train()(xg, kl, mask_padding=True)
    kl[1] = 40
    with pytest.raises(_lib.IsharaError, match="modified in place"):
        (yy * gd).sum().backward()


def test_one_training_step_of_the_model_on_ctc_with_lengths():
    import ishara_amd
    from ishara_amd.squeezeformer import Squeezeformer
    B, T0, F = 3, 150, 24
    m = Squeezeformer(12, F, 64, 3, 1, 3, 2, 2, 2, 0.1, 0.1, 0.1, 0.1, 15, False, seq_len=T0, max_batch=B, dtype="bf16", seed=3).train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, T0, F, generator=g).cuda().requires_grad_(True)
    lens = torch.tensor([150, 120, 90], dtype=torch.int32, device="cuda")
    logp, out_len = m(x, lens, mask_padding=True)
    assert out_len.is_cuda and out_len.tolist() == [17, 13, 9] and logp.shape == (B, 17, 12)
    tgt = torch.randint(1, 12, (B, 4), generator=g)
    loss = ishara_amd.ctc_loss(logp, tgt, out_len, torch.tensor([4, 3, 2]), blank=0, reduction="mean", zero_infinity=True)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
