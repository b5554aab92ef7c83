"""CPU: the references, the length arithmetic, the refusals, the routes and the argument checks of the Squeezeformer family's attention with
per-clip lengths (tests/relattn_len_parity.py; nothing is launched).
  - the operator reference with n = T is r4_parity.relattn_reference, the encoder restatement without lengths is SO.encoder, both to 1e-12 in fp64;
  - the -1e9 fill of the reference equals excluding the keys to 1e-12 (with the n[b] = 0 convention applied to both), and the by-hand backward of
    the flash-style restatement equals autograd;
  - stage_lengths equals SqueezeformerEncoder.output_lengths wherever that is within range and clamps elsewhere, and equals the encoder's own
    stage_lengths method;
  - every refusal of ishara_encoder_forward_lengths / _backward_lengths and of the ishara_relattn_len_* pair, through handles made with device=None;
  - the route names of masked and unmasked calls;
  - SqueezeformerEncoder's argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import r4_parity as R
import relattn_len_parity as L
from ishara_amd import _lib, make_config
from ishara_amd.conformer import ConformerEncoder
from ishara_amd.model import Model
from ishara_amd.squeezeformer import Squeezeformer, SqueezeformerEncoder
from oracle import squeezeformer_torch_oracle as SO

F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
FAKE = C.c_void_p(1 << 20)        # a non-NULL, 256-byte aligned address no refusal dereferences: every call below is refused before any GPU work
OFF2 = C.c_void_p(FAKE.value + 2)
SMALL = [c for c in L.OP_CASES if c[0][2] <= 99]


def _close(a, b, tol=1e-12):
    for k in a:
        s = max(1.0, float(np.abs(a[k]).max()))
        assert float(np.abs(a[k] - b[k]).max()) <= tol * s, (k, float(np.abs(a[k] - b[k]).max()))


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("rate", L.RATES)
@pytest.mark.parametrize("case", [(2, 2, 65, 64), (3, 4, 97, 32), (2, 3, 31, 16)])
def test_full_lengths_are_the_unmasked_reference(case, rate):
    seed = R.dropout_seed(case, rate) if rate > 0 else 4242
    _close(R.relattn_reference(case, "bf16", seed, rate), L.reference(case, (case[2],) * case[0], "bf16", seed, rate))
    _close(R.relattn_reference(case, "bf16", seed, rate), L.reference(case, (case[2] + 5,) * case[0], "bf16", seed, rate))      # clamped to T


@pytest.mark.parametrize("rate", L.RATES)
@pytest.mark.parametrize("case", SMALL, ids=L.case_id)
def test_fill_equals_key_exclusion_and_the_restated_backward_equals_autograd(case, rate):
    shape, n = case
    seed = R.dropout_seed(shape, rate) if rate > 0 else 4242
    a, b = L.reference(shape, n, "bf16", seed, rate), L.reference(shape, n, "bf16", seed, rate, mut=())
    dead = L.dead_clips(shape, n)
    for bb in dead:
        assert (b["lse"][bb] == L.DEAD_LSE).all()
    _close(L.without_dead_lse(a, shape, n), L.without_dead_lse(b, shape, n))


def test_a_dead_clip_is_zero_and_a_masked_key_gets_no_gradient():
    shape, n = L.OP_CASES[2]
    assert n == (97, 0, 1)
    ref = L.reference(shape, n, "f32", 4242, 0.0)
    assert not ref["o"][1].any() and not ref["dq"][1].any() and not ref["dk"][1].any() and not ref["dv"][1].any()
    assert not ref["dv"][2, 1:].any() and ref["dv"][2, 0].any() and not ref["dk"][2, 1:].any()
    assert ref["o"][2].any() and ref["o"][0].any()
    # without the convention the fill averages the padding: the reference's behaviour this library does not follow
    inp = R.relattn_inputs(shape, "f32")
    assert np.abs(inp["v"][1]).max() > 0


@pytest.mark.parametrize("name", sorted(L.ENC_CASES))
def test_the_encoder_restatement_without_lengths_is_the_oracle(name):
    cfg, T0, lens = L.ENC_CASES[name]
    P = SO.init_params(cfg, seed=5, dtype=torch.float64)
    x = torch.randn(len(lens), T0, cfg["input_dim"], generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        for training in (False, True):
            want, _ = SO.encoder(x, P, cfg, training=training)
            got = L.masked_encoder(x, P, cfg, None, training=training)
            assert float((got - want).abs().max()) <= 1e-12
        full = L.masked_encoder(x, P, cfg, (T0,) * len(lens), training=True)
        assert float((full - want).abs().max()) <= 1e-12      # these T0 lose no key to the length arithmetic
        masked = L.masked_encoder(x, P, cfg, lens, training=True)
        assert float((masked[0] - want[0]).abs().max()) > 1e-3      # BatchNorm couples the clips: the full-length clip moves too
        assert float((masked[1] - want[1]).abs().max()) > 1e-2


# ------------------------------------------------------------------ the length arithmetic
@pytest.mark.parametrize("T0,kw", [(150, dict(reduce_layer_index=1, recover_layer_index=3)), (300, dict(reduce_layer_index=1, recover_layer_index=2)),
                                   (800, dict(reduce_layer_index=1, recover_layer_index=2)), (303, dict(reduce_layer_index=3, recover_layer_index=3))])
def test_stage_lengths_follow_output_lengths_and_clamp(T0, kw):
    enc = SqueezeformerEncoder(16, 32, 3, num_attention_heads=2, seq_len=T0, max_batch=2, device=None, **kw)
    T2, T3, Trec = L.stage_dims(T0)
    lens = list(range(-3, T0 + 9))
    n2, n3, nrec = L.stage_lengths(lens, T0)
    m2, m3, mrec = (t.tolist() for t in enc.stage_lengths(torch.tensor(lens)))
    assert (n2, n3, nrec) == (m2, m3, mrec)
    assert max(n2) <= T2 and max(n3) <= T3 and max(nrec) <= Trec and min(n2 + n3 + nrec) == 0
    reduces, recovers = kw["reduce_layer_index"] < 3, kw["recover_layer_index"] < 3
    final = nrec if recovers else (n3 if reduces else n2)
    out = enc.output_lengths(torch.tensor(lens)).tolist()
    hi = Trec if recovers else (T3 if reduces else T2)
    for l, f, o, a in zip(lens, final, out, n2):
        if 0 <= l <= T0 and 0 <= o <= hi and (l >> 2) - 1 >= 0 and ((a >> 1) - 1 >= 0 or not reduces):
            assert f == o, (l, f, o)
    assert n2[lens.index(T0 + 8)] == n2[lens.index(T0)] and n2[lens.index(-3)] == 0
    assert L.stage_lengths([11], 150) == ([1], [0], [0])      # a clip that is dead in the reduced layers only


# ------------------------------------------------------------------ refusals, before any GPU work
def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), msg
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


def test_the_lengths_pair_serves_the_squeezeformer_family_only(lib):
    fwd, bwd = "ishara_encoder_forward_lengths", "ishara_encoder_backward_lengths"
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=2), device=None)
    _refused(lib, lib.ishara_encoder_forward_lengths(m._h, None, 1, None, 0, 0, FAKE, None), fwd, "ISHARA_FAMILY_TORCH_SQUEEZEFORMER", "frame_len", "ishara_forward_ex")
    _refused(lib, lib.ishara_encoder_backward_lengths(m._h, None, 1, None, FAKE, None), bwd, "ISHARA_FAMILY_TORCH_SQUEEZEFORMER", "frame_len")
    enc = ConformerEncoder(32, 1, 4, seq_len=48, max_batch=2, dtype="f32", device=None)
    _refused(lib, lib.ishara_encoder_forward_lengths(enc._h, None, 1, None, 0, 0, FAKE, None), fwd, "ISHARA_FAMILY_TORCH_SQUEEZEFORMER", "key_len", "ishara_encoder_forward_ex")
    _refused(lib, lib.ishara_encoder_backward_lengths(enc._h, None, 1, None, None, None), bwd, "ISHARA_FAMILY_TORCH_SQUEEZEFORMER", "key_len")
    sq = SqueezeformerEncoder(16, 32, 2, 0, 1, 2, seq_len=64, max_batch=2, device=None)
    _refused(lib, lib.ishara_encoder_forward_lengths(sq._h, None, 1, None, 0, 0, OFF2, None), fwd, "misaligned input_len")
    _refused(lib, lib.ishara_encoder_backward_lengths(sq._h, None, 1, None, OFF2, None), bwd, "misaligned input_len")
    _refused(lib, lib.ishara_encoder_forward_lengths(sq._h, None, 1, None, 0, 0, FAKE, None), fwd, "not bound")      # the lengths themselves pass
    _refused(lib, lib.ishara_encoder_forward_lengths(sq._h, None, 1, None, 0, 0, None, None), fwd, "not bound")      # NULL: the plain call's checks
    _refused(lib, lib.ishara_encoder_backward_lengths(sq._h, None, 1, None, FAKE, None), bwd, "not bound")
    # the _ex pair keeps refusing this family (tests/test_attn_mask.py pins the wording)
    _refused(lib, lib.ishara_encoder_forward_ex(sq._h, None, 1, None, 0, 0, None, FAKE, None), "ishara_encoder_forward_ex", "ISHARA_FAMILY_TORCH_CONFORMER")


def test_the_family_has_no_f16_handle(lib):
    """ISHARA_F16 is refused as everywhere in this family: no such handle can be made (ishara_create), so the dtype check of the lengths pair
    is unreachable from outside; the operator pair below refuses the dtype by itself"""
    c = make_config(dim=32, max_batch=2)
    c.family, c.dtype, c.frames, c.features, c.num_heads, c.num_conv_conform_blocks = _lib.FAMILY_TORCH_SQUEEZEFORMER, F16, 64, 16, 2, 2
    c.reduce_layer_index, c.recover_layer_index = 0, 1
    h = C.c_void_p()
    assert lib.ishara_create(C.byref(c), C.byref(h)) != 0 and b"dtype" in lib.ishara_last_error()


OP = dict(B=2, H=2, T=33, dh=16, seed=1, site=2, rate=0.0)


def _op_call(lib, name, dt=F32, key_len=FAKE, route=0, ptrs=None, **kw):
    a = {**OP, **kw}
    n = 9 if name.endswith("fwd") else 14
    p = list(ptrs) if ptrs is not None else [FAKE] * n
    return getattr(lib, name)(dt, *p, a["B"], a["H"], a["T"], a["dh"], a["seed"], a["site"], C.c_float(a["rate"]), key_len, route, FAKE, None)


@pytest.mark.parametrize("name", ["ishara_relattn_len_fwd", "ishara_relattn_len_bwd"])
def test_the_operator_pair_makes_the_parent_checks_then_its_own(lib, name):
    _refused(lib, _op_call(lib, name, dt=F16), name, "ISHARA_F16")
    _refused(lib, _op_call(lib, name, dt=7), name, "unknown dtype")
    _refused(lib, _op_call(lib, name, dh=12), name, "head dim")
    _refused(lib, _op_call(lib, name, T=0), name, ">= 1")
    _refused(lib, _op_call(lib, name, rate=1.0), name, "rate")
    n = 9 if name.endswith("fwd") else 14
    _refused(lib, _op_call(lib, name, ptrs=[None] + [FAKE] * (n - 1)), name, "null or misaligned buffer")
    _refused(lib, _op_call(lib, name, ptrs=[OFF2] + [FAKE] * (n - 1)), name, "null or misaligned buffer")
    _refused(lib, _op_call(lib, name, key_len=None), name, "key_len")
    _refused(lib, _op_call(lib, name, key_len=OFF2), name, "misaligned key_len")
    _refused(lib, _op_call(lib, name, route=2), name, "route")
    # the same messages as the pair without lengths, the name apart
    parent = name.replace("ishara_relattn_len_", "ishara_op_relattn_")
    for kw in (dict(dh=12), dict(T=0), dict(rate=1.0)):
        a = {**OP, **kw}
        getattr(lib, parent)(F32, *([FAKE] * n), a["B"], a["H"], a["T"], a["dh"], a["seed"], a["site"], C.c_float(a["rate"]), FAKE, None)
        want = lib.ishara_last_error().decode().replace(parent, name)
        _op_call(lib, name, **kw)
        assert lib.ishara_last_error().decode() == want
    assert lib.ishara_relattn_len_scratch_bytes(2, 2, 33, 12) < 0 and lib.ishara_relattn_len_scratch_bytes(2, 2, 0, 16) < 0
    assert lib.ishara_relattn_len_scratch_bytes(2, 2, 33, 16) == lib.ishara_op_relattn_scratch_bytes(2, 2, 33, 16) > 0


# ------------------------------------------------------------------ routes
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("dh", [8, 16, 32, 64])
@pytest.mark.parametrize("T", [1, 99, 198, 199])
def test_route_names(lib, dt, dh, T):
    name = lambda bwd, masked: lib.ishara_debug_relattn_kernel_name(dt, bwd, T, dh, masked).decode()
    assert name(0, 0) == "relattn_len_fwd_kernel"                                  # the call without lengths: the lane kernels, at every dtype and head dim
    assert name(1, 0) == "relattn_len_bwd_dq_kernel+relattn_len_bwd_dkv_kernel+relattn_len_bwd_dpos_kernel"
    mfma = dt == BF16 and dh in (32, 64)      # the MFMA forward: bf16 at head dim 32 / 64, any T
    assert name(0, 1) == ("relattn_len_fwd_mfma_kernel" if mfma else "relattn_len_fwd_kernel")
    assert name(1, 1) == "relattn_len_bwd_dq_kernel+relattn_len_bwd_dkv_kernel+relattn_len_bwd_dpos_kernel"


def test_refused_routes_have_no_name(lib):
    for masked in (0, 1):
        assert lib.ishara_debug_relattn_kernel_name(F16, 0, 99, 64, masked) == b""
        assert lib.ishara_debug_relattn_kernel_name(BF16, 0, 99, 40, masked) == b""
        assert lib.ishara_debug_relattn_kernel_name(BF16, 1, 0, 64, masked) == b""


# ------------------------------------------------------------------ the Python arguments (no device: every one raises before any)
@pytest.fixture(scope="module")
def enc():
    return SqueezeformerEncoder(16, 32, 2, 0, 1, 2, seq_len=64, max_batch=2, device=None)


def test_mask_padding_needs_lengths(enc):
    with pytest.raises(ValueError, match="input_lengths"):
        enc(torch.zeros(2, 64, 16), mask_padding=True)
    with pytest.raises(TypeError):
        enc(torch.zeros(2, 64, 16), torch.tensor([64, 30]), True)      # keyword only


@pytest.mark.parametrize("bad", [torch.zeros(2, 2, dtype=torch.int32), torch.tensor([64.0, 29.0]), torch.tensor([True, False]), 5, np.zeros((2, 1), np.int64)])
def test_lengths_that_are_no_integer_vector_are_refused(enc, bad):
    with pytest.raises(ValueError, match="input_lengths"):
        enc(torch.zeros(2, 64, 16), bad, mask_padding=True)


def test_the_model_passes_the_keyword_on():
    m = Squeezeformer(10, 16, 32, 2, 0, 1, 2, seq_len=64, max_batch=2, device=None)
    with pytest.raises(ValueError, match="input_lengths"):
        m(torch.zeros(2, 64, 16), torch.tensor([64.0, 29.0]), mask_padding=True)
