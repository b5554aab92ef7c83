"""GPU: the A-stationary GEMM family (gemm_as.hip, gemm_as_f16.hip) through ishara_op_gemm_as — one launch_gemm_nt call on a caller-built weight
shadow of exactly N rows, nothing but the GEMM kernel in the launch sequence — against the int64 / fp64 reference of tests/gemm_as_parity.py, at the
row-form, ring, column-split, paired-store and chunked-kernel edges test_gemm_as_plan.py shows the table to contain.

Every case without Swish or a LayerNorm prologue runs in the exact form: array_equal on C, pre_out (whole [M, ldc] buffers: the gap columns and the
columns past n_valid must still hold the sentinel), q, k, vt and pro_out after one rounding to the output type, the sentinels around every output
untouched.  Every case that is no fingerprint also runs real-valued: the derived worst-case bound of fp32 summation, TOL for the Swish cases, and for
the LayerNorm prologue the two checks of gemm_as_parity.py (statistics and pro_out against fp64 LayerNorm under the derived bound plus the measured
reciprocal-square-root allowance; the GEMM against the product of the device's own pro_out).  One launch per case and form.

A failure of an exact case names, for the first wrong elements, (m, n), the workgroup, pass, wave, row tile, column step and ring slot, got and
want, and for a fingerprint case the step's or row's weights and the row's activations.  Each real-valued test prints its worst error / bound ratio
before it asserts (pytest -s); DESIGN.md section 2 records them."""
import numpy as np
import pytest

import gemm_as_parity as G

pytestmark = pytest.mark.gpu


def _expected(dev, c, real):
    """reference and bound with the dropout mask ishara_dropout_mask draws for the call's seed / site / rate (cases without one: the cached ones)"""
    if not c.drop:
        return G.expected(c.name, real)
    op, masks = G.inputs(c.name, real), dev.masks()
    cpu = G.cpu_masks(c)
    assert all(np.array_equal(masks[k], cpu[k]) for k in masks), "ishara_dropout_mask and its oracle mirror disagree"
    return G.reference(c, op, masks, rounded=not real), (G.bounds(c, op, masks) if real else None)


def _plan_line(c):
    p = G.plan(c.name)
    return f"{p.route} {p.kernel} rows {p.rows} grid ({p.gx}, {p.gy}) nsteps {p.nsteps} hold {p.hold}"


@pytest.mark.parametrize("name", [c.name for c in G.EXACT_CASES])
def test_case_exact(lib, name):
    c = G.BY_NAME[name]
    assert G.lib_plan(lib, c) == G.plan(name)
    dev = G.Device(lib, c, G.inputs(name, False))
    ref, _ = _expected(dev, c, False)
    got = dev.launch()
    assert got["guards_ok"], f"{name}: a sentinel in front of or behind an output was written"
    assert set(ref) == set(got) - {"guards_ok"}
    wrong = [G.describe_wrong(c, n, got[n], ref[n]) for n in ref if not np.array_equal(got[n].astype(np.float64), ref[n])]
    print(f"gemm_as_parity exact {name} {_plan_line(c)} {'equal' if not wrong else 'WRONG'}")
    assert not wrong, f"{name}: differs from the exact reference\n" + "\n".join(wrong)


@pytest.mark.parametrize("name", [c.name for c in G.REAL_CASES if c.pro != "ln"])
def test_case_real_valued(lib, name):
    c = G.BY_NAME[name]
    dev = G.Device(lib, c, G.inputs(name, True))
    ref, bound = _expected(dev, c, True)
    got = dev.launch()
    assert got["guards_ok"], f"{name}: a sentinel in front of or behind an output was written"
    ratio = G.worst_ratio(c, got, ref, bound)
    print(f"gemm_as_parity real {name} {_plan_line(c)} err/{'TOL' if c.real_only else 'bound'} " + " ".join(f"{n}={v:.3g}" for n, v in ratio.items()))
    over = {n: v for n, v in ratio.items() if not v <= 1.0}
    assert not over, f"{name}: error over the {'tolerance' if c.real_only else 'derived bound'} (ratio): {over}"


@pytest.mark.parametrize("name", [c.name for c in G.LN_CASES])
def test_case_layernorm_prologue(lib, name):
    c = G.BY_NAME[name]
    assert G.lib_plan(lib, c) == G.plan(name)
    op = G.inputs(name, True)
    dev = G.Device(lib, c, op)
    masks = dev.masks()
    got = dev.launch()
    assert got["guards_ok"], f"{name}: a sentinel in front of or behind an output was written"
    plain = c._replace(real_only=False)
    # (1) the prologue against fp64 LayerNorm
    ln = G.ln_reference(c, op)
    side = [n for n in ("ln_mean", "ln_rstd", "pro_out") if n in got]
    assert side == ((["ln_mean", "ln_rstd"] if c.stats else []) + (["pro_out"] if c.pro_out else []))
    r1 = G.worst_ratio(plain, got, {n: ln[n][0] for n in side}, {n: ln[n][1] for n in side})
    if "ln_rstd" in got:
        rel = float((np.abs(got["ln_rstd"].astype(np.float64) - ln["ln_rstd"][0]) / ln["ln_rstd"][0]).max())
        print(f"gemm_as_parity ln {name} worst |ln_rstd - rstd| / rstd = {rel:.4g} (allowance {G.RSQ_ALLOW:.4g})")
    # (2) the GEMM against the product of the DEVICE's pro_out (the reference's own where the case asks for none: the bound then carries the
    # operand's rounding, one ulp of the operand type on every product)
    if c.pro_out:
        a = got["pro_out"].astype(np.float64)
        ref, bound = G.reference(c, op, masks, rounded=False, a_staged=a), G.bounds(c, op, masks, a_staged=a)
    else:
        ref, bound = G.reference(c, op, masks, rounded=False), G.bounds(c, op, masks)
        y_b = G.ln_reference(c, op)["pro_out"][1]
        extra = y_b @ np.abs(op["W"]).T
        for n in bound:
            bound[n] = bound[n] + (extra if n in ("C", "pre_out") else 0.0)
    main = [n for n in ref if n != "pro_out"]
    r2 = G.worst_ratio(plain, got, {n: ref[n] for n in main}, {n: bound[n] for n in main})
    print(f"gemm_as_parity ln {name} {_plan_line(c)} prologue err/bound " + " ".join(f"{n}={v:.3g}" for n, v in r1.items()) + " | gemm err/bound "
          + " ".join(f"{n}={v:.3g}" for n, v in r2.items()))
    over = {n: v for n, v in {**r1, **r2}.items() if not v <= 1.0}
    assert not over, f"{name}: error over the derived bound (ratio): {over}"
