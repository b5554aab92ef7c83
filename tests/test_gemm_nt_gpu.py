"""GPU: the three tile kernels of gemm_nt.hip through ishara_op_gemm_nt (one launch_gemm_nt call on a caller-built weight shadow: nothing but the
GEMM kernel in the launch sequence) against the int64 / fp64 reference of tests/gemm_nt_parity.py, at the tile, ring and persistent-round edges
test_gemm_nt_plan.py shows the table to contain.

Every case runs in the exact form (array_equal on C, pre_out, q, k, vt after one rounding to dtC; the sentinels around every output untouched;
NaN in the discarded rows of Bt not leaking) and, fingerprint cases apart, real-valued (the derived worst-case bound of fp32 summation; TOL for the
Swish cases).  The persistent and fingerprint cases of the 128 x 128 tile kernel also run five times into five fresh output buffers, every launch
compared with the exact reference; the shape of DESIGN.md section 4's open item (M = 34816, K = 640, N = 768, residual) runs five times more
through ishara_op_dense_fwd_ex, with the operator's shadow rebuild in the sequence, on the same integer operands and the same reference.

A failure of an exact case names, for the first wrong elements, (m, n), the output tile, for NT_TILE_T the tile id, workgroup and round, got and
want, and for a fingerprint case the K-tile digits.  Each real-valued test prints its worst error / bound ratio before it asserts (pytest -s);
DESIGN.md section 2 records them per route."""
import ctypes as C

import numpy as np
import pytest

import gemm_nt_parity as G
from ishara_amd import _lib

pytestmark = pytest.mark.gpu

REPEATS = 5


def _expected(dev, c, real):
    """reference and bound with the dropout masks ishara_dropout_mask draws for the call's seed / site / rate (cases without one: the cached ones)"""
    if not (c.drop or c.op == "dropmask"):
        return G.expected(c.name, real)
    op, masks = G.inputs(c.name, real), dev.masks()
    cpu = G.cpu_masks(c)
    assert all(np.array_equal(masks[k], cpu[k]) for k in masks), "ishara_dropout_mask and its oracle mirror disagree"
    return G.reference(c, op, masks, rounded=not real), (G.bounds(c, op, masks) if real else None)


def _check_exact(label, c, got, ref):
    assert got["guards_ok"], f"{label}: a sentinel in front of or behind an output was written"
    wrong = [G.describe_wrong(c, n, got[n], ref[n]) for n in ref if not np.array_equal(got[n].astype(np.float64), ref[n])]
    print(f"gemm_nt_parity exact {label} {'equal' if not wrong else 'WRONG'}")
    assert not wrong, f"{label}: differs from the exact reference\n" + "\n".join(wrong)


@pytest.mark.parametrize("name", [c.name for c in G.EXACT_CASES])
def test_case_exact(lib, name):
    c = G.BY_NAME[name]
    assert G.route(lib, c) == (c.route, G.kernel_name(c))
    dev = G.Device(lib, c, G.inputs(name, False))
    ref, _ = _expected(dev, c, False)
    _check_exact(f"{name} {c.route}", c, dev.launch(), ref)


@pytest.mark.parametrize("name", [c.name for c in G.RUN_CASES if not c.fp])
def test_case_real_valued(lib, name):
    c = G.BY_NAME[name]
    dev = G.Device(lib, c, G.inputs(name, True))
    ref, bound = _expected(dev, c, True)
    got = dev.launch()
    assert got["guards_ok"], f"{name}: a sentinel in front of or behind an output was written"
    ratio = G.worst_ratio(c, got, ref, bound)
    print(f"gemm_nt_parity real {name} {c.route} {G.kernel_name(c)} err/{'TOL' if c.real_only else 'bound'} " + " ".join(f"{n}={v:.3g}" for n, v in ratio.items()))
    over = {n: v for n, v in ratio.items() if not v <= 1.0}
    assert not over, f"{name}: error over the {'tolerance' if c.real_only else 'derived bound'} (ratio): {over}"


@pytest.mark.parametrize("name", [c.name for c in G.REPEAT_CASES])
def test_persistent_and_fingerprint_cases_five_fresh_launches(lib, name):
    c = G.BY_NAME[name]
    dev = G.Device(lib, c, G.inputs(name, False))
    ref, _ = _expected(dev, c, False)
    failures = []
    for i in range(REPEATS):
        try:
            _check_exact(f"{name} launch {i}", c, dev.launch(), ref)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_reported_shape_five_times_through_the_dense_operator(lib):
    """the shape of the open item through ishara_op_dense_fwd_ex: memset + make_shadow_kernel + GEMM per call, as the test that reported it ran.
    A failure here alone points at the shadow rebuild; one in test_persistent_and_fingerprint_cases_five_fresh_launches[t_reported] too, at the kernel.

    Observed on the MI355X (the open item): this test passed when the file ran alone and failed once in a whole-suite run, at
    launch 0 of the 5 — 16 wrong elements of 26 738 688, rows 576.. of column 636 only, tile (4, 4), id 36, workgroup 36, round 0 (that
    workgroup's FIRST tile), got - want = -2, -1, +6, -8, -4, +7, ...: one accumulator register (acc[3][0][0] of wave (1, 1)) in one quarter of the
    lanes.  Launches 1 .. 4 of that run and all launches on the caller-built shadow were exact.  A later whole-suite run saw the same register wrong in
    test_case_exact[t_reported], the first launch of the shape in the process, on the caller-built shadow (tile (20, 0), workgroup 100, round 0, rows 2624 ..
    of column 124): the shadow rebuild is not needed for it.  The cause is not found; the test keeps asserting."""
    import torch
    c = G.BY_NAME[G.REPORTED]
    op = G.inputs(c.name, False)
    ref, _ = G.expected(c.name, False)

    def up(x, dt):
        return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dt).cuda()

    x, W, b, r = up(op["A"], torch.bfloat16), up(op["W"].T, torch.float32), up(op["bias"], torch.float32), up(op["resid"], torch.bfloat16)
    sc, scp = _lib.aligned(int(lib.ishara_op_scratch_bytes(c.M, c.K, c.N)), "cuda")
    failures = []
    try:
        lib.ishara_debug_force_regstage(G.FORCE[c.route])
        assert lib.ishara_debug_dense_kernel_name(_lib.BF16, c.M, c.K, c.N, 0, 1) == G.kernel_name(c).encode()
        for i in range(REPEATS):
            y = torch.full((c.M, c.N), G.SENTINEL["bf16"], dtype=torch.bfloat16, device="cuda")
            _lib.check(lib.ishara_op_dense_fwd_ex(_lib.BF16, _lib.ptr(x), _lib.ptr(W), _lib.ptr(b), _lib.ptr(r), _lib.ptr(y), c.M, c.K, c.N, 0, scp, _lib.stream()), "ishara_op_dense_fwd_ex")
            torch.cuda.synchronize()
            got = y.float().cpu().numpy()
            if not np.array_equal(got.astype(np.float64), ref["C"]):
                failures.append(G.describe_wrong(c, "C", got, ref["C"]).replace(c.name, f"{c.name} dense_fwd_ex launch {i}"))
    finally:
        lib.ishara_debug_force_regstage(0)
    print(f"gemm_nt_parity exact {c.name} dense_fwd_ex x{REPEATS} {'equal' if not failures else 'WRONG'}")
    assert not failures, "\n".join(failures)
