"""CPU: the case table of tests/gemm_as_parity.py contains what it is for.  The plan of every case — route, profiler key, rows per workgroup, grid,
column steps, ring depth, steps per stage, waves, passes, chunked, paired stores, compiled mask, prologue — comes from ishara_debug_gemm_as_plan,
i.e. from gemm_nt_as_plan, the function run_as launches from (host only, nothing is launched), and must equal the plan the table computes for the
row.  Every listed edge must hold for the cases that claim it — computed from the shape and that plan, not from the row's label — and must have a
case; the exact form's preconditions (every intermediate an integer below 2^24, every stored 16-bit operand representable) hold for every case."""
import numpy as np
import pytest

import gemm_as_parity as G


@pytest.fixture(scope="module")
def plans(lib):
    return {c.name: G.lib_plan(lib, c) for c in G.CASES}


def test_every_case_runs_on_the_plan_its_row_claims(plans):
    wrong = [(c.name, plans[c.name], G.plan(c.name)) for c in G.CASES if plans[c.name] != G.plan(c.name)]
    assert not wrong, wrong[:5]
    assert {p.route for p in plans.values()} == {"NT_AS", "NT_AS_F16"}
    assert {c.name for c in G.CASES if plans[c.name].route == "NT_AS_F16"} == {c.name for c in G.CASES if c.dt == "f16"}


def test_every_compiled_instantiation_has_a_case(plans):
    """(operand type, C type, prologue) -> the compiled masks the table reaches must be the lists run_as switches over"""
    seen = {}
    for c in G.CASES:
        if c.K in (256, 512):
            seen.setdefault((c.dt, c.dtC, c.pro, c.K), set()).add(plans[c.name].inst)
    for K in (256, 512):
        assert seen[("bf16", "bf16", "none", K)] == set(G.BF16_MASKS) | {G.ALL}
        assert seen[("f16", "f16", "none", K)] >= set(G.F16_MASKS)
        assert seen[("bf16", "bf16", "ln", K)] >= set(G.LN_MASKS)
    assert seen[("bf16", "f32", "none", 256)] | seen[("bf16", "f32", "none", 512)] == {0, G.ALL}
    assert seen[("f16", "f32", "none", 256)] | seen[("f16", "f32", "none", 512)] == {0, G.ALL}
    assert G.ALL in seen[("f16", "f16", "none", 256)]
    assert seen[("bf16", "bf16", "pa", 256)] == set(G.PA_MASKS) == seen[("bf16", "bf16", "pa", 512)]
    assert {plans[c.name].inst for c in G.CASES if c.K == 128} == {G.M_DACT, G.M_DACT | G.DROP, G.ALL}
    # the profiler keys name the kernels: chunked and per-step, with and without a prologue
    keys = {p.kernel for p in plans.values()}
    assert "gemm_nt_as_chunk_kernel<bf16,8,0,0>" in keys and "gemm_nt_as_chunk_kernel<bf16,16,1,0>" in keys and "gemm_nt_as_chunk_kernel<bf16,8,0,1>" in keys
    assert "gemm_nt_as_kernel<bf16,8,0,0>" in keys and "gemm_nt_as_kernel<f32,16,255,0>" in keys and "gemm_nt_as_kernel<bf16,16,17,0,2>" in keys
    assert "gemm_nt_as_kernel<bf16,32,0,0>" in keys and "gemm_nt_as_kernel<bf16,4,2,0>" in keys and "gemm_nt_kernel<f16>" in keys


def test_the_fallbacks_of_the_chunked_kernel(plans):
    for name in ("chunk_not_split", "chunk_not_n_valid", "chunk_not_stages", "chunk_not_flag"):
        p = plans[name]
        assert not p.chunked and p.cs == 1 and p.ring == 3 and p.kernel.startswith("gemm_nt_as_kernel<"), (name, p)
    assert plans["chunk_not_split"].gy == 2 and plans["chunk_not_split"].nsteps == 4
    on = [c.name for c in G.CASES if plans[c.name].chunked]
    assert len(on) >= 12 and all(plans[n].gy == 1 and plans[n].rows == 384 and plans[n].kernel.startswith("gemm_nt_as_chunk_kernel<bf16,") for n in on)


def test_no_case_needs_the_c_stationary_switches(lib, plans):
    """as_flags never carries bits 6 / 7: K = 512, N = 256 would leave the family under them, and the entry says so by the route's name"""
    assert all(c.as_flags & 192 == 0 for c in G.CASES)
    c = G.case("cs_shape", 49536, 256, 512, "x", resid=True, as_flags=51 | 192)
    G.BY_NAME[c.name] = c
    try:
        p = G.lib_plan(lib, c)
        assert p.route == "NT_REFUSED" and "route NT_CS" in lib.ishara_last_error().decode()
        G.BY_NAME[c.name] = c._replace(as_flags=51)
        assert G.lib_plan(lib, G.BY_NAME[c.name]).route == "NT_AS"
    finally:
        del G.BY_NAME[c.name]


def test_every_case_has_the_edges_it_is_listed_for():
    wrong = [(c.name, p) for c in G.CASES for p in c.props if not G.PROPS[p](c)]
    assert not wrong, wrong
    assert all(c.props for c in G.CASES)


def test_every_edge_has_a_case():
    have = {p for c in G.CASES for p in c.props}
    assert have == set(G.PROPS), (sorted(set(G.PROPS) - have), sorted(have - set(G.PROPS)))


def test_every_mistake_has_cases_it_applies_to():
    for mut in G.MUTANTS:
        assert [c.name for c in G.EXACT_CASES if G.mutant_applies(c, mut)], mut


def test_the_shared_inputs_of_the_paired_store_rows():
    groups = {}
    for c in G.CASES:
        if c.like != c.name:
            groups.setdefault(c.like, []).append(c)
    assert len(groups) == 8
    for like, cs in groups.items():
        base = G.BY_NAME[like]
        assert sorted(c.as_flags for c in cs + [base]) == sorted(G.FLAGS)
        assert all(c._replace(name="", as_flags=0, like="", props=()) == base._replace(name="", as_flags=0, like="", props=()) for c in cs)
        assert G.inputs(cs[0].name, False) is G.inputs(like, False)


TYPE_OF = {"A": "dt", "W": "dt", "aux": "dtC", "resid": "dtC"}


@pytest.mark.parametrize("name", [c.name for c in G.EXACT_CASES])
def test_exact_form_stays_below_2_to_the_24(name):
    c = G.BY_NAME[name]
    op = G.inputs(name, False)
    masks = G.cpu_masks(c)
    for n, x in op.items():
        assert np.array_equal(G.store(x, getattr(c, TYPE_OF[n]) if n in TYPE_OF else "f32"), x), (name, n)
        if not c.fp:
            assert np.array_equal(x, np.rint(x)), (name, n)
    A = G.staged(c, op)
    assert np.array_equal(A, G.store(A, c.dt)) and (c.fp or np.array_equal(A, np.rint(A)))          # the transformed operand is a value of the operand type
    if c.pro == "pa":
        b = np.arange(c.M) // c.T
        assert np.array_equal(A, op["A"] * op["P"][b] + op["Q"][b]) and np.abs(A).max() <= 256          # ... with no rounding at all
        assert set(np.unique(np.abs(op["P"]))) <= {1.0, 2.0} and len(op["P"]) == G.nsamples(c) > 1 and not np.array_equal(op["P"][0], op["P"][1])
    mag = G.magnitudes(c, op, masks)
    worst = max(float(np.abs(v).max()) for v in mag.values())
    assert worst < 2.0 ** 24, (name, worst)
    ref = G.compute(c, op, masks)
    for n, v in ref.items():          # no output reaches the sentinel, 16-bit outputs stay finite
        assert np.abs(v).max() < G.SENTINEL[c.dt if n == "pro_out" else c.dtC], (name, n)
    if c.fp:
        assert c.dtC == "bf16" and not c.bias and ref["C"].max() <= 256 and np.array_equal(ref["C"], np.rint(ref["C"])) and np.array_equal(G.store(ref["C"], "bf16"), ref["C"])
    if c.rowscale:
        assert set(np.unique(op["rowscale"])) <= {1.0, 2.0, 4.0} and len(set(op["rowscale"][:3])) == 3
    assert c.act in ("none", "relu") and c.dact in ("none", "pos") and c.pro in ("none", "pa")


def test_fingerprints_name_step_weight_row_and_activations():
    for name in ("fp_step_k256", "fp_lane_k512", "fp_step_chunk"):
        c = G.BY_NAME[name]
        ref = G.expected(name, False)[0]["C"]
        for m, n in ((0, 0), (1, 33), (c.M - 1, c.N - 1), (64, 70)):
            own = n // 32 if c.fp == "step" else n % 32
            assert ref[m, n] == int(G.fp_row_factor(m)) * (1 + own)
            assert G.decode(c, ref[m, n], m, n) == {"weights": own, "a": int(G.fp_row_factor(m))}, (name, m, n)
        assert G.decode(c, float("nan"), 0, 0) == {"weights": None, "a": None} and G.decode(c, 0.0, 0, 0) == {"weights": None, "a": None}
    a = G.fp_row_factor(np.arange(5000))
    assert set(a) == {1, 2, 3} and (a[1:] != a[:-1]).all()          # neighbouring rows always differ


def test_locate_follows_the_kernels_row_and_column_split():
    c = G.BY_NAME["k512_m32769"]                 # 192-row workgroups: a 128-row pass of 32 rows per wave, then a 64-row pass of 16
    assert G.locate(c, 192 * 3 + 127, 0) == dict(x=3, y=0, ps=0, wave=3, tile=1, step=0, slot=0, sub=0)
    assert G.locate(c, 192 * 3 + 128 + 17, 31) == dict(x=3, y=0, ps=1, wave=1, tile=0, step=0, slot=0, sub=0)
    c = G.BY_NAME["k256_n2_split"]               # N = 1024 over 16 splits of 2 steps
    assert G.locate(c, 5, 64 * 7 + 40) == dict(x=0, y=7, ps=0, wave=0, tile=0, step=1, slot=1, sub=0)
    c = G.BY_NAME["fp_step_chunk"]               # 12 waves of 32 rows, stages of 4 steps, two slots
    assert G.locate(c, 384 * 2 + 32 * 11 + 16, 32 * 6 + 1) == dict(x=2, y=0, ps=0, wave=11, tile=1, step=6, slot=1, sub=2)
    c = G.BY_NAME["k256_n5"]                     # ring of 3: step 3 is back in slot 0
    assert G.locate(c, 70, 32 * 3)["slot"] == 0 and G.locate(c, 70, 32 * 4)["slot"] == 1
