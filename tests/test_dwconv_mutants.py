"""CPU: what tests/test_dwconv_bwd_gpu.py can and cannot miss.  The case list of tests/dwconv_parity.py reaches every backward route and every
instantiation of the one-pass kernel; the fp64 restatement of the one-pass arrangement (segments, preloaded halo, "newest row" dbias rule)
equals the autograd reference; restated with ideal bf16 rounding it stays inside the bf16 bounds (no bound asks for more than the format
gives); and each ordinary mistake, switched on alone, exceeds a bound by 2x or more in f32 and in bf16, the seam and halo mistakes as an
integer mismatch on the counting inputs."""
import itertools

import numpy as np
import pytest

import dwconv_parity as D

ONE_PASS = [c for c in D.CASES if c.kernel in (D.FUSED, D.FUSED_BN)]


def find(group, dtype, **kw):
    hits = [c for c in D.CASES if c.group == group and c.dtype == dtype and all(getattr(c, k) == v for k, v in kw.items())]
    assert hits, (group, dtype, kw)
    return hits[0]


def test_every_case_names_the_kernel_the_route_picks(lib):
    wrong = [(D.case_id(c), D.expected_kernel(lib, c)) for c in D.CASES if D.expected_kernel(lib, c) != c.kernel]
    assert not wrong, wrong[:5]


def _kind(name):
    """kernel name -> route class: the tile kernel's <KC,KM> variants are one data-gradient kind"""
    for t in (D.TILE11, D.TILE15, D.TILE31):
        name = name.replace(t, "dwconv_kernel")
    return name


def _grid(lib):
    """(dt, C, k, padl, scratch, bn, force) -> kernel name over everything the route looks at"""
    for dt, Cc, k, pc, scr, bn, force in itertools.product((D.F32, D.BF16), (8, 24, 128, 256, 1000, 1024, 1152, 2048), range(1, 32), "cs0", (0, 1), (0, 1), (0, 1)):
        lib.ishara_debug_force_regstage(D.FORCE_LDS if force else 0)
        name = lib.ishara_debug_dwconv_kernel_name(dt, 1, 2, 64, Cc, k, D.pad(pc, k), (D.SCR if scr else 0) | (D.BN if bn else 0)).decode()
        yield (dt, Cc, k, bn), name
    lib.ishara_debug_force_regstage(0)


def test_cases_reach_every_route_and_every_one_pass_instantiation(lib):
    try:
        grid = list(_grid(lib))
    finally:
        lib.ishara_debug_force_regstage(0)
    # every DwBwdKind x DwDgrad x DwWgrad combination the route returns anywhere on the grid
    reachable = {_kind(n) for _, n in grid if n}
    assert len(reachable) == 6, reachable      # one-pass with / without BatchNorm, reg + atomic, tile + win / part / atomic
    assert {_kind(c.kernel) for c in D.CASES} == reachable
    # every <dtype, K, INOP, WU, BN> of the one-pass kernel a call can land on (the input op takes no part in the route)
    dts = {D.F32: "f32", D.BF16: "bf16"}
    want = {(dts[dt], k, inop, (Cc // 4) % 64 == 0, n == D.FUSED_BN) for (dt, Cc, k, bn), n in grid if n in (D.FUSED, D.FUSED_BN) for inop in (0, 1, 2)}
    assert len(want) == 3 * 2 * ((4 + 3) + (2 + 2)), len(want)      # bf16 K 3 5 11 15 (+ BatchNorm: 3 5 11), f32 K 3 5 (both)
    have = {(c.dtype, *D.fused_variant(c)) for c in ONE_PASS}
    assert have == want, sorted(want - have)


RESTATED = [c for i, c in enumerate(ONE_PASS) if c.group in ("fused-T", "fused-op", "fused-samples", "bn-T", "bn-auto", "bn-k15") and (i % 3 == 0 or c.T > 64)]


def test_restatement_equals_the_reference():
    assert len(RESTATED) > 80
    for c in RESTATED:
        op = D.inputs(c)
        ref, got = D.reference(c, op), D.restate(c, op, start=(0.0, 0.0))
        if c.consistent:      # dx of these is autograd through the BatchNorm itself: equal up to the fp32 rounding of the coefficients and of h
            assert D.act_metrics(got["dx"], ref["dx"])[0] < (2e-2 if c.dtype == "bf16" else 1e-5), D.case_id(c)
            ref.pop("dx")
        for n in ref:
            assert np.abs(got[n] - ref[n]).max() <= 1e-9 * max(1.0, np.abs(ref[n]).max()), (D.case_id(c), n)


def test_bf16_bounds_are_capped():
    assert all(v <= D.BF16_CAP for q, v in D.BF16_BOUND.items() if q.endswith("_l2"))


def test_ideal_bf16_restatement_stays_inside_the_bounds():
    """fp64 with the BatchNorm-transformed row and dx rounded to bf16 once, every sum exact: the least any bf16 kernel can do"""
    for c in RESTATED:
        if c.dtype != "bf16":
            continue
        op = D.inputs(c)
        got = D.restate(c, op, ideal_bf16=True, start=(0.0, 0.0))
        if not c.bias:
            got.pop("dbias")
        over = D.excess(D.observe(c, got, D.reference(c, op)), D.bounds(c))
        assert not over, (D.case_id(c), over)


def _mutant_case(mut, dtype):
    """the listed case a mistake is switched on in: T = 33 (one step past the first 32-step segment), k = 5"""
    if mut in ("halo_zero", "seam_twice"):
        return find("fused-T", dtype, k=5, T=65, padl=4)
    if mut == "halo_prev_sample":
        return find("fused-T", dtype, k=5, T=33, padl=2)
    if mut == "swish_sigma_only":
        return find("fused-op", dtype, k=5, inop=D.SWISH, bias=True)
    if mut == "glu_no_1ms":
        return find("fused-op", dtype, k=5, inop=D.GLU, bias=True)
    if mut.startswith("bn_"):
        return find("bn-T", dtype, k=5, T=33, bn="block")
    return find("fused-T", dtype, k=5, T=33, padl=4)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mut", D.MUTANTS)
def test_each_mistake_exceeds_a_bound_twice_over(mut, dtype):
    c = _mutant_case(mut, dtype)
    op = D.inputs(c)
    ref = D.reference(c, op)
    start = dict(dx=0.0, dw=D.DW_START, dbias=D.DBIAS_START)

    def figures(m):
        got = D.restate(c, op, mut=m, ideal_bf16=dtype == "bf16")
        got = {n: (D._round(got[n], dtype) if n == "dx" else np.asarray(got[n], np.float32).astype(np.float64)) - start[n] for n in ref}
        return D.observe(c, got, ref)

    bound = D.bounds(c)
    assert not D.excess(figures(()), bound), "the restatement without a mistake is outside the bounds"
    obs = figures((mut,))
    ratio = max(obs[q] / b for q, b in bound.items() if q in obs)
    assert ratio >= 2.0, (mut, D.case_id(c), obs, bound)


@pytest.mark.parametrize("mut", ["halo_zero", "halo_prev_sample", "seam_twice", "dbias_drop_head", "dw_tail"])
def test_counting_inputs_reject_seam_and_halo_mistakes_exactly(mut):
    c = _mutant_case(mut, "bf16")
    op = D.counting_inputs(c)
    want = D.counting_expect(c, op["w"])
    clean = D.restate(c, op, start=(0.0, 0.0), inop=D.NONE)
    assert all(np.array_equal(clean[n], want[n]) for n in want), "the counting expectation disagrees with the restatement"
    got = D.restate(c, op, mut=(mut,), start=(0.0, 0.0), inop=D.NONE)
    diff = np.concatenate([(got[n] - want[n]).ravel() for n in want])
    assert np.abs(diff).max() >= 0.25 and np.array_equal(diff * 4, np.round(diff * 4)), "not an integer mismatch"
