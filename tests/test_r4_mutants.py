"""CPU: the bounds of tests/test_ops_r4_gpu.py reject ordinary mistakes.  Each mistake below is applied to the fp64 reference of an operator
(r4_parity's restatements) on the inputs the GPU test draws, the mutant's tensors are rounded to the storage dtype as a kernel's would be, and
compared with the clean reference through the GPU test's own compare(): at least one asserted quantity must exceed its bound by 2x, in f32
and in bf16 — a kernel making that mistake cannot pass.  Also: the restatements compute what the oracle's functions do when nothing is
switched on."""
import numpy as np
import pytest

import module_parity as MP
import r4_parity as R

RELATTN_SHAPES = [(3, 4, 97, 32), (2, 2, 65, 64)]
# mistake -> dropout rate it needs
RELATTN_MUTANTS = {
    "row_off": 0.0,              # table row T-i+j instead of T-1-i+j
    "swap_uv": 0.0,              # u_bias in the positional score, v_bias in the content score
    "dposp_batch0": 0.0,         # dposp not summed over the batch
    "mask_not_in_bwd": R.RATE,   # the mask applied in the forward pass but not to dP
    "mask_no_head": R.RATE,      # the mask row key b*T + i
    "du_no_scale": 0.0,          # du without the softmax scale
    "delta_undropped": R.RATE,   # delta from the undropped output
}
ROUNDED = ("o", "dq", "dk", "dv", "sub", "red", "dh")      # tensors a kernel stores in the storage dtype


def _round(out, dtype):
    return {k: (MP.round_to(v, dtype).astype(np.float64) if k in ROUNDED else v) for k, v in out.items() if k != "alts"}


def _worst_ratio(obs, bound):
    r = {}
    for key, v in obs.items():
        n, q = key.rsplit(".", 1)
        b = bound["zero"]["zero"] if q == "zero" else bound.get(n, {}).get(q)
        if b is not None:
            r[key] = v / b
    return max(r.values()), r


@pytest.mark.parametrize("rate", [0.0, R.RATE])
@pytest.mark.parametrize("case", RELATTN_SHAPES + [(2, 2, 1, 8)])
def test_unmutated_attention_restatement_is_the_oracle(case, rate):
    seed = R.dropout_seed(case, rate) if rate > 0 else 4242
    a, b = R.relattn_reference(case, "bf16", seed, rate), R.relattn_reference(case, "bf16", seed, rate, mut=())
    for k in a:
        assert np.allclose(a[k], b[k], rtol=1e-10, atol=1e-11), k


@pytest.mark.parametrize("case", R.SUB_CASES[:3])
def test_unmutated_subsampling_restatement_is_the_oracle(case):
    a, b = R.subsample_reference(case, "bf16"), R.subsample_reference(case, "bf16", mut=())
    for k in b:
        if k != "alts":
            assert np.allclose(a[k], b[k], rtol=1e-12, atol=1e-12), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", RELATTN_SHAPES, ids=lambda c: "B%d-H%d-T%d-dh%d" % c)
@pytest.mark.parametrize("mut", sorted(RELATTN_MUTANTS))
def test_bounds_reject_the_attention_mutant(mut, case, dtype):
    rate = RELATTN_MUTANTS[mut]
    seed = R.dropout_seed(case, rate) if rate > 0 else 4242
    ref = R.relattn_reference(case, dtype, seed, rate)
    bad = _round(R.relattn_reference(case, dtype, seed, rate, mut=(mut,)), dtype)
    bound = R.bounds(dtype)
    obs, _ = R.compare(bad, ref, bound, case[0] * case[2])
    worst, ratios = _worst_ratio(obs, bound)
    print(mut, case, dtype, {k: f"{v:.1f}x" for k, v in ratios.items() if v >= 1})
    assert worst >= 2.0, f"{mut}: no asserted quantity exceeds 2x its {dtype} bound: {ratios}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.SUB_CASES[1:3], ids=lambda c: "B%d-T%d-F%d-d%d" % c)
@pytest.mark.parametrize("mut", ["gate_on_dsub", "w2_transposed"])
def test_bounds_reject_the_subsampling_mutant(mut, case, dtype):
    ref = R.subsample_reference(case, dtype)
    bad = _round(R.subsample_reference(case, dtype, mut=(mut,)), dtype)
    bound = R.bounds(dtype)
    _, _, T2, F2 = R.sub_dims(case[1], case[2])
    obs, _ = R.compare(bad, ref, bound, case[0] * T2 * F2, ref["alts"])
    worst, ratios = _worst_ratio(obs, bound)
    print(mut, case, dtype, {k: f"{v:.1f}x" for k, v in ratios.items() if v >= 1})
    assert worst >= 2.0, f"{mut}: no asserted quantity exceeds 2x its {dtype} bound: {ratios}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.TRED_CASES[1:3], ids=lambda c: "B%d-T%d-d%d" % c)
@pytest.mark.parametrize("mut", ["ignore_extra", "w_transposed"])
def test_bounds_reject_the_time_reduction_mutant(mut, case, dtype):
    ref = R.tred_reference(case, dtype, True)
    bad = _round(R.tred_reference(case, dtype, True, mut=(mut,)), dtype)
    bound = R.bounds(dtype)
    obs, _ = R.compare(bad, ref, bound, case[0] * R.tred_dims(case[1], case[2])[0])
    worst, ratios = _worst_ratio(obs, bound)
    print(mut, case, dtype, {k: f"{v:.1f}x" for k, v in ratios.items() if v >= 1})
    assert worst >= 2.0, f"{mut}: no asserted quantity exceeds 2x its {dtype} bound: {ratios}"
