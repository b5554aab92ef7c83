"""CPU: the bounds of tests/test_relattn_len_gpu.py reject the mistakes a length-aware attention kernel can make.  Each mistake is applied to the
fp64 restatement (relattn_len_parity.reference / masked_encoder) on the inputs the GPU test draws, the mutant's stored tensors are rounded to the
storage dtype as a kernel's would be, and compared with the clean reference through the GPU test's own comparison: at least one asserted
quantity must exceed its bound by 2x, in f32 and in bf16.  The factor is printed."""
import numpy as np
import pytest

import r4_parity as R
import relattn_len_parity as L
from test_r4_mutants import _worst_ratio

SHAPES = [L.OP_CASES[2], L.OP_CASES[1], L.OP_CASES[4]]      # a dead and a one-key clip; T = QB + 1 at dh 64; a short first clip
# mistake -> dropout rate it needs
MUTANTS = {
    "len_ignored": 0.0,          # every key attended
    "len_le": 0.0,               # j <= n instead of j < n
    "len_on_queries": 0.0,       # the lengths applied to the query rows
    "len_not_in_bwd": 0.0,       # the backward recomputes P over every key
    "mask_no_head": R.RATE,      # dropout keyed by b*T + i
    "row_off": 0.0,              # the positional window one row off, under a mask
}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", SHAPES, ids=L.case_id)
@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_bounds_reject_the_operator_mutant(mut, case, dtype):
    shape, n = case
    rate = MUTANTS[mut]
    seed = R.dropout_seed(shape, rate) if rate > 0 else 4242
    ref = L.reference(shape, n, dtype, seed, rate)
    bad = L.rounded(L.reference(shape, n, dtype, seed, rate, mut=(mut,)), dtype)
    bound = L.op_bounds(shape, n, dtype, seed, rate, mfma=dtype == "bf16" and shape[3] in (32, 64))      # the wider of the two routes' bounds
    obs, _ = L.compare(bad, ref, bound, shape, n)
    worst, ratios = _worst_ratio(obs, bound)
    print(mut, L.case_id(case), dtype, {k: f"{v:.1f}x" for k, v in ratios.items() if v >= 1})
    assert worst >= 2.0, f"{mut}: no asserted quantity exceeds 2x its {dtype} bound: {ratios}"


def test_the_storage_restatement_stays_inside_its_own_bound():
    """op_bounds never falls below r4_parity's and holds the restatement it was derived from, with the margin of 2"""
    for shape, n in L.OP_CASES[:5]:
        b = L.op_bounds(shape, n, "bf16", 4242, 0.0)
        for name, qs in R.BF16_BOUND.items():
            for q, v in qs.items():
                assert b[name][q] >= v
        ref = L.reference(shape, n, "bf16", 4242, 0.0)
        st = L.rounded(L.reference(shape, n, "bf16", 4242, 0.0, mut=("bf16_storage",)), "bf16")
        _, bad = L.compare(st, ref, b, shape, n)
        assert not bad, bad


def encoder_errors(y, dx, grads, ref_y, ref_dx, ref_grads):
    """the quantities tests/test_relattn_len_gpu.py asserts at encoder level: y max-abs, dx (max over max, rel-L2), the worst parameter gradient
    (max over max, rel-L2)"""
    out = dict(y=float(np.abs(y - ref_y).max()), dx_max=float(np.abs(dx - ref_dx).max() / np.abs(ref_dx).max()),
               dx_l2=float(np.linalg.norm(dx - ref_dx) / np.linalg.norm(ref_dx)))
    gscale = max(float(np.abs(v).max()) for v in ref_grads.values())
    gm, gl = 0.0, 0.0
    for k, want in ref_grads.items():
        if np.abs(want).max() < 1e-6 * gscale:
            continue
        gm = max(gm, float(np.abs(grads[k] - want).max() / np.abs(want).max()))
        if want.size > 16:
            gl = max(gl, float(np.linalg.norm(grads[k] - want) / np.linalg.norm(want)))
    out.update(grad_max=gm, grad_l2=gl)
    return out


# f32: test_squeezeformer_other_shapes_vs_oracle's; bf16: test_squeezeformer_training_pass_matches_reference_autograd's, the output's raised per
# case by relattn_len_parity.encoder_y_bound
ENC_BOUND = {"f32": dict(y=2e-4, dx_max=2e-3, grad_max=3e-3), "bf16": dict(y=0.1, dx_l2=0.12, grad_l2=0.12)}


@pytest.mark.parametrize("mut", ["n2_in_reduced", "lengths_ignored"])
@pytest.mark.parametrize("name", sorted(L.ENC_CASES))
def test_bounds_reject_the_encoder_mutant(name, mut):
    _, _, P, y, dx = L.encoder_reference(name)
    grads = {k: v.grad.numpy().copy() for k, v in P.items() if v.grad is not None}
    if mut == "lengths_ignored":
        _, _, Pm, ym, dxm = L.encoder_reference(name, with_lengths=False)
    else:
        _, _, Pm, ym, dxm = L.encoder_reference(name, mut=(mut,))
    gm = {k: v.grad.numpy() for k, v in Pm.items() if v.grad is not None}
    e = encoder_errors(ym.numpy(), dxm.numpy(), gm, y.numpy(), dx.numpy(), grads)
    for dtype, bound in ENC_BOUND.items():
        bound = dict(bound, y=L.encoder_y_bound(name)) if dtype == "bf16" else bound
        ratios = {q: e[q] / b for q, b in bound.items()}
        print(name, mut, dtype, {q: f"{v:.1f}x" for q, v in ratios.items()})
        assert max(ratios.values()) >= 2.0, (dtype, ratios)
