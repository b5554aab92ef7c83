"""CPU: the case table of tests/gemm_nt_parity.py contains what it is for.  Route and profiler key of every case come from
ishara_debug_gemm_nt_route, i.e. from gemm_nt_route — the function launch_gemm_nt launches from (host only, nothing is launched).  Every listed
edge must hold for the cases that claim it — computed from M, N, K, the route's tile and K-tile sizes and the 768-workgroup grid, not from the
row's label — and must have a case; the exact form's precondition (every intermediate an integer below 2^24) holds for every case; the refused
rows are refused."""
import numpy as np
import pytest

import gemm_nt_parity as G


@pytest.fixture(scope="module")
def routes(lib):
    return {c.name: G.route(lib, c) for c in G.CASES}


def test_every_case_runs_on_the_route_and_kernel_its_row_claims(routes):
    wrong = [(c.name, routes[c.name]) for c in G.RUN_CASES if routes[c.name] != (c.route, G.kernel_name(c))]
    assert not wrong, wrong
    assert {c.route for c in G.CASES} == {"NT_TILE_T", "NT_GLDS", "NT_REG"}
    # every instantiation the three kernels are compiled for, once at least
    want = {f"gemm_nt_{k}_kernel<{t}>" for k in ("t", "glds") for t in ("f32,f32", "bf16,bf16", "bf16,f32")}
    want |= {"gemm_nt_kernel<f32,f32,f32>", "gemm_nt_kernel<bf16,bf16,bf16>", "gemm_nt_kernel<f32,bf16,bf16>", "gemm_nt_kernel<bf16,bf16,f32>", "gemm_nt_kernel<f16>"}
    assert {k for _, k in routes.values()} - {""} == want


def test_the_default_route_takes_the_cases_that_claim_it(lib):
    """force = False rows run with no switch set; the others need theirs (the default route would be another kernel or the same one)"""
    free = [c for c in G.RUN_CASES if not c.force]
    assert {c.route for c in free} == {"NT_TILE_T", "NT_GLDS", "NT_REG"}
    for c in free:
        assert G.route(lib, c._replace(force=True))[0] == c.route, c.name          # (the route's own switch selects it too)
    # the reported shape runs on the 256 x 256 kernel by default, which this entry does not serve: the switch is what puts it on the tile kernel
    rep = G.BY_NAME[G.REPORTED]
    assert G.route(lib, rep._replace(force=False)) == ("NT_REFUSED", "") and b"NT_BIG" in lib.ishara_last_error()
    assert G.route(lib, rep) == ("NT_TILE_T", "gemm_nt_t_kernel<bf16,bf16>")


def test_every_case_has_the_edges_it_is_listed_for():
    wrong = [(c.name, p) for c in G.CASES for p in c.props if not G.PROPS[p](c)]
    assert not wrong, wrong
    assert all(c.props for c in G.CASES)


def test_every_edge_has_a_case():
    have = {p for c in G.CASES for p in c.props}
    assert have == set(G.PROPS), (sorted(set(G.PROPS) - have), sorted(have - set(G.PROPS)))


def test_the_epilogue_variant_of_the_tile_kernel_is_what_the_rows_are_for():
    by_ek = {e: [c.name for c in G.RUN_CASES if c.route == "NT_TILE_T" and G.ek(c) == e] for e in (0, 1, 2)}
    assert all(len(v) >= 8 for v in by_ek.values()), by_ek
    # persistent shapes: more than 768 tiles, under 100 MB of operands and outputs, on each epilogue variant
    pers = [c for c in G.RUN_CASES if c.route == "NT_TILE_T" and G.ntiles(c) > G.GRID and c.name != G.REPORTED]
    assert {G.ek(c) for c in pers} == {0, 1, 2}
    for c in pers:
        es = {"f32": 4, "bf16": 2}
        moved = c.M * c.K * es[c.dtA] + c.M * c.N * es[c.dtC] * (2 if c.resid else 1)
        assert moved < 100e6, (c.name, moved)
    assert {c.name for c in G.REPEAT_CASES} >= {c.name for c in pers} | {G.REPORTED, "t_fpW", "t_fpA"}


def _max_magnitude(c, op, masks):
    """an upper bound of every |partial sum| and |epilogue intermediate| of the case from sums of absolute values: the largest row sum of one
    operand times the largest element of the other, then the epilogue's addends and scales at their largest"""
    A, W = G.staged(c, op, masks, absolute=True), np.abs(op["W"])
    v = min(A.sum(1).max() * W.max(), A.max() * W.sum(1).max())
    rs = float(np.abs(op["rowscale"]).max()) if c.rowscale else 1.0
    if c.bias:
        v += np.abs(op["bias"]).max() * rs
    if c.tab:
        v += np.abs(op["addtab"]).max()
    v *= (2.0 if c.drop else 1.0) * rs
    if c.resid:
        v += np.abs(op["resid"]).max()
    return v


@pytest.mark.parametrize("name", [c.name for c in G.EXACT_CASES])
def test_exact_form_stays_below_2_to_the_24(name):
    c = G.BY_NAME[name]
    op = G.inputs(name, False)
    masks = G.cpu_masks(c)
    for n, x in op.items():
        assert np.array_equal(G.store(x, c.dtC if n in ("aux", "resid") else (c.dtA if n == "A" else (c.dtM if n == "W" else "f32"))), x), (name, n)
        if not c.fp:
            assert np.array_equal(x, np.rint(x)), (name, n)
    A = G.staged(c, op, masks)
    assert np.array_equal(A, G.store(A, c.dtM))
    if c.fp:
        assert G.nk(c) <= 8 and c.dtC == "f32" and c.K % G.bk(c) == 0
    assert _max_magnitude(c, op, masks) < 2.0 ** 24, name
    if c.rowscale:
        assert set(np.unique(op["rowscale"])) <= {1.0, 2.0, 4.0} and len(set(op["rowscale"][:3])) == 3
    assert c.act in ("none", "relu") and c.dact in ("none", "pos")


def test_fingerprints_decode_to_one_digit_per_k_tile():
    for name in ("t_fpW", "t_fpA", "g_fpW", "g_fpA_f32"):
        c = G.BY_NAME[name]
        ref = G.expected(name, False)[0]["C"]
        for m in (0, 1, c.M - 1):
            a = 1 if c.fp == "W" else int(G.fp_row_factor(m))
            assert G.decode(ref[m, c.N - 1], G.nk(c)) == [a] * G.nk(c), (name, m)
    assert G.decode(8.0 ** 8, 8) is None and G.decode(-1.0, 8) is None and G.decode(1.5, 8) is None and G.decode(float("nan"), 8) is None


def test_tile_mapping_round_trips():
    for c in G.RUN_CASES:
        ids = {G.tile_id(c, mt, nt) for mt in range(G.n_mt(c)) for nt in range(G.n_nt(c))} if G.ntiles(c) < 4000 else None
        if ids is not None:
            assert ids == set(range(G.ntiles(c))), c.name
        for tid in (0, G.ntiles(c) - 1, G.ntiles(c) // 2):
            assert G.tile_id(c, *G.tile_of(c, tid)) == tid


def test_refused_rows_are_refused(lib, routes):
    for c in G.CASES:
        assert (routes[c.name][0] == "NT_REFUSED") == c.refused, c.name
        if c.refused:
            assert routes[c.name] == ("NT_REFUSED", "")
            G.route(lib, c)
            msg = lib.ishara_last_error().decode()
            assert msg.startswith("ishara_debug_gemm_nt_route:"), msg
            want = {"rowscale": "OP_ROWSCALE"}.get(c.op, "f16 operands take no operand transform" if c.dtM == "f16" else "A rows must be 16-byte aligned")
            assert want in msg, (c.name, msg)
    assert G.route(lib, G.BY_NAME["t_nk1"])[0] == "NT_TILE_T"          # the switch was restored, the entry still answers
