"""GPU: the weight-gradient GEMM family through ishara_op_gemm_tn (launch_gemm_tn as the models' gemm_wgrad calls it) against the int64 / fp64
reference of tests/gemm_tn_parity.py, at the split and tile edges test_gemm_tn_plan.py shows the table to contain.

Every case runs in the exact form (array_equal on out, dbias, G, Rpart; the guard regions behind them untouched) and real-valued (the derived
worst-case bound of fp32 summation), each with its M-split sums taken at once and through the deferred-sum state, and, where the route allows,
on the forced register-transposing kernel.  The chains run several calls through ONE deferred-sum state — riders, a call that sums at once, a
call on another kernel, the per-sample-affine kernel's inline sums, the big-tile kernel's flush, the final flush — and every output of every
call must be exact.  One chain runs five times with bit-identical results.

Each test prints its worst error / bound ratios before it asserts (pytest -s); DESIGN.md section 2 records them per route."""
import numpy as np
import pytest

import gemm_tn_parity as G

pytestmark = pytest.mark.gpu

MODES = [("exact", False), ("real", True)]


@pytest.fixture(scope="module")
def slabs(lib):
    import torch
    need = max(G.slab_bytes(lib, [c]) for c in G.RUN_CASES)
    return [torch.empty(need // 4, dtype=torch.float32, device="cuda") for _ in range(3)]


def _check(label, c, real, got, op):
    ref, bound = G.expected(c.name, real)
    assert set(ref) <= set(got)
    assert got["guards_ok"], f"{label}: a guard region behind an output was written"
    if not real:
        wrong = {n: int((got[n].astype(np.float64) != ref[n]).sum()) for n in ref if not np.array_equal(got[n].astype(np.float64), ref[n])}
        print(f"gemm_tn_parity exact {label} mismatching elements {wrong or 0}")
        assert not wrong, f"{label}: elements that differ from the exact reference: {wrong}"
        return
    ratio = G.worst_ratio(got, ref, bound)
    print(f"gemm_tn_parity real {label} err/bound " + " ".join(f"{n}={v:.3g}" for n, v in ratio.items()))
    over = {n: v for n, v in ratio.items() if not v <= 1.0}
    assert not over, f"{label}: error over the derived bound (ratio): {over}"


@pytest.mark.parametrize("deferred", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("mode,real", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("name", [c.name for c in G.RUN_CASES])
def test_case_against_reference(lib, slabs, name, mode, real, deferred):
    c = G.BY_NAME[name]
    op = G.inputs(name, real)
    got = G.run(lib, [(c, op)], deferred, slabs)[0]
    _check(f"{name} {G.plan(lib, c).route} {'deferred' if deferred else 'immediate'}", c, real, got, op)


@pytest.mark.parametrize("deferred", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("mode,real", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("name", [c.name for c in G.FORCED])
def test_forced_register_kernel_against_reference(lib, slabs, name, mode, real, deferred):
    c = G.BY_NAME[name]
    assert G.plan(lib, c, force=True).route == "TN_REG"
    op = G.inputs(name, real)
    got = G.run(lib, [(c, op)], deferred, slabs, force=True)[0]
    _check(f"{name} TN_REG forced {'deferred' if deferred else 'immediate'}", c, real, got, op)


@pytest.mark.parametrize("mode,real", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("chain", sorted(G.CHAINS))
def test_deferred_chain_every_output_of_every_call(lib, slabs, chain, mode, real):
    items = [(G.BY_NAME[n], G.inputs(n, real)) for n in G.CHAINS[chain]]
    got = G.run(lib, items, True, slabs)
    failures = []
    for i, ((c, op), g) in enumerate(zip(items, got)):
        try:
            _check(f"chain {chain} call {i} {c.name}", c, real, g, op)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures


def test_chain_is_bit_identical_run_to_run(lib, slabs):
    items = [(G.BY_NAME[n], G.inputs(n, True)) for n in G.CHAINS["riders"]]
    first = G.run(lib, items, True, slabs)
    for _ in range(4):
        again = G.run(lib, items, True, slabs)
        for a, b in zip(first, again):
            for n in a:
                if n != "guards_ok":
                    assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n
