"""CPU: the bounds of tests/test_attn_gpu.py reject ordinary mistakes, and are not below what bf16 allows.  Each mistake below is applied to
attn_parity.restate, the fp64 restatement of the flash algorithm the kernels follow, on the inputs the GPU test draws at its edge shapes; the
mutant's o, dq, dk, dv are rounded to the storage dtype as a kernel's would be and compared with the clean reference through the GPU test's own
compare(): at least one asserted quantity must exceed its bound by 2x, in f32 and in bf16 — a kernel making that mistake cannot pass.  Also: with
nothing switched on the restatement is the reference; the restatement with the MFMA kernels' bf16 roundings stays inside BF16_BOUND; the seeds
the GPU test uses draw masks with the share of zeros it asserts; the closed forms of the q = 0 regime and the ordering of the late / early
regimes hold."""
import math

import numpy as np
import pytest
import torch

import attn_parity as A
import module_parity as MP

C = A.Case
# the shapes the mistakes are applied at: past one query block and off the key chunk of the route (MFMA: 128 / 64, lane-split: 64 / 32)
SHAPES = {"bf16": [C("mfma", "bf16", 1, 3, 136, 32, 0.0, 0, False, A.MAIN), C("mfma", "bf16", 1, 3, 200, 32, 0.0, 0, False, A.MAIN)],
          "f32": [C("lane", "f32", 2, 3, 65, 24, 0.0, 0, False, A.MAIN), C("lane", "f32", 2, 3, 130, 8, 0.0, 0, False, A.MAIN)]}
# mistake -> (dropout rate it needs, score regime)
MUTANTS = {
    "keys_past_T_unmasked": (0.0, A.MAIN),          # the loads clamp to row T-1: that key is counted again for every key >= T of the last chunk
    "vt_past_T_not_zeroed": (0.0, A.MAIN),          # with those keys unmasked (a masked key multiplies whatever V^T holds there by 0)
    "acc_not_rescaled": (0.0, "late"),              # the running maximum rises in every chunk
    "lse_without_max": (0.0, A.MAIN),
    "o_without_keep_scale": (A.RATE, A.MAIN),
    "mask_not_in_dP": (A.RATE, A.MAIN),
    "mask_not_in_dV": (A.RATE, A.MAIN),
    "mask_no_head": (A.RATE, A.MAIN),               # row key b*T + i
    "mask_qblock0": (A.RATE, A.MAIN),               # the mask rows of query block 0 for every query block
    "delta_from_undropped_o": (A.RATE, A.MAIN),
    "dS_without_scale": (0.0, A.MAIN),
    "dk_first_query_block_only": (0.0, A.MAIN),
    "q_k_columns_swapped": (0.0, A.MAIN),
}


def _rounded(out, dtype, c, mut=()):
    """o, dq, dk, dv as stored; delta as a kernel forms it, from the stored o (unless the mistake is to take it from elsewhere)"""
    out = {k: (MP.round_to(v, dtype).astype(np.float64) if k in A.ROUNDED else v) for k, v in out.items()}
    if "delta_from_undropped_o" not in mut:
        out["delta"] = A.delta_from(out["o"], A.inputs(c)[1], A.shape(c))
    return out


def _compare(c, got):
    """as the GPU test compares: delta against rowsum(dO o o) of the (mutant's) own o"""
    ref = dict(A.reference(c))
    if np.isfinite(got["o"]).all():
        ref["delta"] = A.delta_from(got["o"], A.inputs(c)[1], A.shape(c))
    return A.compare(got, ref, A.bounds(c))


def _worst_ratio(obs, bad, bound):
    if any("not finite" in b for b in bad):
        return math.inf, {}
    r = {}
    for key, v in obs.items():
        n, q = key.rsplit(".", 1)
        b = bound["zero"]["zero"] if q == "zero" else bound[n].get(q)
        if b is not None:
            r[key] = v / b
    return max(r.values()), r


@pytest.mark.parametrize("c", [c._replace(rate=r, dm=2 if r else 0, regime=g) for cs in SHAPES.values() for c in cs for r, g in ((0.0, A.MAIN), (A.RATE, A.MAIN), (0.0, "late"))]
                         + [C("lane", "bf16", 2, 3, 1, 16, A.RATE, 1, False, A.MAIN)], ids=A.case_id)
def test_unmutated_restatement_is_the_reference(c):
    a, b = A.reference(c), A.restate(c)
    for k in a:
        assert np.allclose(a[k], b[k], rtol=1e-10, atol=1e-11), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_bounds_reject_the_mutant(mut, dtype):
    rate, regime = MUTANTS[mut]
    for base in SHAPES[dtype]:
        if mut in ("mask_qblock0", "dk_first_query_block_only") and base.T <= A.QB[base.route]:
            continue
        c = base._replace(rate=rate, dm=(2 if base.route == "mfma" else 1) if rate else 0, regime=regime)
        assert rate == 0 or A.mask_of(A.shape(c), A.seed_of(c), rate) is not None
        obs, bad = _compare(c, _rounded(A.restate(c, mut=(mut,)), dtype, c, (mut,)))
        worst, ratios = _worst_ratio(obs, bad, A.bounds(c))
        print(mut, A.case_id(c), {k: f"{v:.1f}x" for k, v in ratios.items() if v >= 1} or bad)
        assert worst >= 2.0, f"{mut} at {A.case_id(c)}: no asserted quantity exceeds 2x its {dtype} bound: {ratios}"
        obs, bad = _compare(c, _rounded(A.restate(c), dtype, c))
        assert not bad, f"the clean restatement fails at {A.case_id(c)}: {bad}"


# every MFMA case once (the forced two-kernel backward and DM 1 round alike) and the bf16 T = 1 cases, whose dq and dk are the zero bound's
BF16_MFMA = [c for c in A.CASES if c.route == "mfma" and not c.two_pass and c.dm != 1] + [c for c in A.CASES if c.dtype == "bf16" and c.T == 1]


@pytest.mark.parametrize("c", BF16_MFMA, ids=A.case_id)
def test_ideal_bf16_restatement_is_within_the_bf16_bounds(c):
    """the algorithm with exactly the MFMA kernels' roundings and exact sums: a bound below its error would ask for more than the format gives"""
    obs, bad = _compare(c, A.restate(c, ideal_bf16=True))
    print(A.case_id(c), {k: f"{v:.3g}" for k, v in obs.items()})
    assert not bad, "\n".join(bad)
    # whatever is measured: the cap on every rel-L2 bound must leave room for the format's own error, with the 2x of the rule to spare
    assert all(v <= MP.BF16_CAP / 2 for k, v in obs.items() if k.endswith(".l2")), obs


def test_bf16_bounds_are_capped():
    """every bf16 tensor has a rel-L2 bound, none above 0.03; lse and delta have an elem bound and the analytic zeros a bound of their own"""
    for bb in [A.BF16_BOUND, *A.BF16_REGIME_BOUND.values()]:
        for b in bb.values():
            assert all(v is None or v > 0 for v in b.values())
            assert "l2" not in b or 0.0 < b["l2"] <= MP.BF16_CAP
    assert all(A.BF16_BOUND[n]["l2"] is not None for n in A.TENSORS)
    assert A.BF16_BOUND["lse"]["elem"] and A.BF16_BOUND["delta"]["elem"] and A.BF16_BOUND["zero"]["zero"]


def test_chosen_seeds_draw_the_mask_share_the_gpu_test_asserts():
    seen = 0
    for c in A.CASES:
        if c.rate > 0 and c.B * c.H * c.T * c.T >= 4096:
            lo, hi = A.mask_share_range(c.rate)
            share = float((A.mask_of(A.shape(c), A.seed_of(c), c.rate) == 0).double().mean())
            assert lo <= share <= hi, (A.case_id(c), share)
            seen += 1
    assert seen > 50 and A.mask_share_range(A.RATE) == (0.10, 0.30)
    assert A.mask_of(A.shape(A.TINY_RATE_CASE), 4242, A.TINY_RATE_CASE.rate) is None      # thr8 = 0: no mask at all


def test_case_list_reaches_every_backward_instantiation(lib):
    kernels = {A.bwd_kernel(lib, c) for c in A.CASES}
    for nw, nt in ((8, 1), (12, 1), (8, 2), (12, 2)):
        for dm in (0, 1, 2):
            for form in ("FULL", "ragged"):
                assert f"attn_bwd_fused_kernel<{nw},{nt},{dm},{form}>" in kernels
    for dh in (32, 64):
        for dm in (0, 1, 2):
            assert f"attn_bwd_dq_mfma_kernel + attn_bwd_dkv_mfma_kernel<{dh},{dm}>" in kernels
    for dt in ("float", "bf16"):
        for dhl in (2, 4, 6, 8, 12, 16):
            assert f"attn_bwd_dq_kernel + attn_bwd_dkv_kernel<{dt},{dhl}>" in kernels
    assert len({A.case_id(c) for c in A.CASES}) == len(A.CASES)


@pytest.mark.parametrize("route,T,dh", [("mfma", 136, 32), ("mfma", 136, 64), ("lane", 65, 16)])
def test_score_regimes_are_what_they_are_named(route, T, dh):
    B, H = (1, 3) if route == "mfma" else (2, 3)
    kc = A.KC[route]
    for regime in ("late", "early", "q0"):
        c = C(route, "bf16", B, H, T, dh, 0.0, 0, False, regime)
        qkv, _ = A.inputs(c)
        x = torch.from_numpy(qkv).double().view(B, T, H, 3 * dh).permute(0, 2, 1, 3)
        s = x[..., :dh] @ x[..., dh:2 * dh].transpose(-1, -2) * A.scale_of(c)
        ref = A.reference(c)
        if regime == "q0":
            v = x[..., 2 * dh:].mean(2)      # [B, H, dh]
            assert np.allclose(ref["lse"], math.log(T), rtol=0, atol=1e-12)
            assert np.allclose(ref["o"].reshape(B, T, H, dh), v.numpy()[:, None], rtol=0, atol=1e-12)
            continue
        chunk = s.argmax(-1) // kc
        assert bool((chunk == ((T - 1) // kc if regime == "late" else 0)).all())
        # per chunk maxima are at least 20 apart, in the order the regime names; "early": the last chunk lies more than 88 below the maximum
        mx = torch.stack([s[..., k0:k0 + kc].max(-1).values for k0 in range(0, T, kc)], -1)
        step = (mx[..., 1:] - mx[..., :-1]) * (1 if regime == "late" else -1)
        assert float(step.min()) > 20.0
        if regime == "early":
            assert float((mx[..., 0] - mx[..., -1]).min()) > 88.0
