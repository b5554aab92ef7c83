"""CPU: the comparison tests/test_param_groups_gpu.py applies to the grouped step and the mask (param_groups_parity.compare /
compare_mask) accepts the reference and rejects the ordinary mistakes, each restated in numpy on the parity cases: lr_scale ignored, the
row of a neighbouring segment, the first or last element of a segment under the neighbour's row, the last element of a chunk skipped, a
frozen segment's m or v advanced, wd * 0 computed as upd + 0 * theta on the Inf weight, `skipped` counted once per workgroup; a mask that
writes -0.0, leaves a NaN or zeroes the wrong segment."""
import numpy as np
import pytest

import param_groups_parity as PG
from ishara_amd import train_state as TS


def _step(c, iteration, lr, wd, coef, decay_always=False):
    """one plain step of the whole vector in numpy -> (theta, m, v, slow); decay_always: upd + wd * theta also when wd == 0"""
    st = dict(m=c["m"].copy(), v=c["v"].copy(), slow=c["slow"].copy(), step=iteration - 1, skipped=0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if decay_always and wd == 0.0:
            k = TS.radam_coeffs(iteration)
            g = c["grad"] * np.float32(coef)
            m = 0.9 * st["m"] + (1 - 0.9) * g
            v = 0.999 * st["v"] + (1 - 0.999) * g * g
            mh = m * np.float32(k["c1"])
            upd = np.float32(k["r_t"]) * mh / (np.sqrt(v * np.float32(k["c2"])) + np.float32(1e-7)) if k["rect"] else mh
            upd = upd + np.float32(0.0) * c["theta"]
            th = c["theta"] - np.float32(lr) * upd
            slow = st["slow"]
            if iteration % 5 == 0:
                slow = slow + np.float32(0.5) * (th - slow)
                th = slow.copy()
            return th.astype(np.float32), m.astype(np.float32), v.astype(np.float32), slow.astype(np.float32)
        th = TS.clipped_step_reference(c["theta"].copy(), c["grad"], st, lr, coef=coef, weight_decay=wd)
    return th, st["m"], st["v"], st["slow"]


def _mutant(name, assignment, iteration, variant="plain", *, ignore_lr_scale=False, row_shift=0, edge=None, skip_chunk_last=False,
            frozen_moves=None, decay_always=False, skipped_per_workgroup=False):
    """the grouped step with the chosen mistakes -> a result as param_groups_parity.compare takes it"""
    c = PG.vectors(name, assignment, variant)
    seg = [int(o) for o in PG.table(name)]
    rows = PG.rows(name, assignment)
    S = len(rows)
    coef, nonfinite, skipped = c["rec"] if c["rec"] else (1.0, 0, 0)
    out = {k: c[k].copy() for k in ("theta", "m", "v", "slow")}
    if c["skip"] and nonfinite > 0:
        groups = min(TS.GRAD_GRID_CAP, sum(-(-(hi - lo) // PG.CHUNK) for lo, hi in zip(seg[:-1], seg[1:])))
        return dict(out, rec=(coef, nonfinite, skipped + (groups if skipped_per_workgroup else 1)))
    runs = {}

    def run(r):
        lr = np.float32(PG.LR) * (np.float32(1.0) if ignore_lr_scale else r["lr_scale"])
        wd = np.float32(PG.WD) * r["wd_scale"]
        key = (lr.tobytes(), wd.tobytes())
        if key not in runs:
            runs[key] = _step(c, iteration, float(lr), float(wd), coef, decay_always)
        return runs[key]

    def put(r, idx):
        if r["frozen"]:
            if frozen_moves:                                    # the slot advances although the segment is frozen
                k = {"m": 1, "v": 2}[frozen_moves]
                out[frozen_moves][idx] = run(rows[0])[k][idx]
            return
        for k, a in zip(("theta", "m", "v", "slow"), run(r)):
            out[k][idx] = a[idx]

    for s in range(S):
        lo, hi = seg[s], seg[s + 1]
        put(rows[min(max(s + row_shift, 0), S - 1)], slice(lo, hi))
        if edge == "first" and s > 0:
            for k in out:
                out[k][lo] = c[k][lo]
            put(rows[s - 1], slice(lo, lo + 1))
        if edge == "last" and s + 1 < S:
            for k in out:
                out[k][hi - 1] = c[k][hi - 1]
            put(rows[s + 1], slice(hi - 1, hi))
        if skip_chunk_last:
            for e in list(range(lo + PG.CHUNK - 1, hi, PG.CHUNK)) + [hi - 1]:
                for k in out:
                    out[k][e] = c[k][e]
    return dict(out, rec=(coef, nonfinite, skipped) if c["rec"] else None)


@pytest.mark.parametrize("name,assignment,variant", PG.CASES)
def test_the_comparison_accepts_the_reference_and_a_faithful_restatement(name, assignment, variant):
    for it in PG.ITERATIONS:
        exp = PG.expected(name, assignment, it, variant)
        assert PG.compare(exp, exp) == []
        assert PG.compare(_mutant(name, assignment, it, variant), exp) == [], it


@pytest.mark.parametrize("iteration", PG.ITERATIONS)
@pytest.mark.parametrize("assignment", ["cycle", "shifted", "ends"])
@pytest.mark.parametrize("mistake,needle", [
    (dict(ignore_lr_scale=True), "theta"),
    (dict(row_shift=1), "theta"),
    (dict(row_shift=-1), "theta"),
    (dict(edge="first"), "theta"),
    (dict(edge="last"), "theta"),
    (dict(skip_chunk_last=True), "m"),
    (dict(frozen_moves="m"), "m"),
    (dict(frozen_moves="v"), "v"),
])
def test_the_comparison_rejects(mistake, needle, assignment, iteration):
    for name in ("A", "C", "D"):
        bad = PG.compare(_mutant(name, assignment, iteration, **mistake), PG.expected(name, assignment, iteration))
        assert any(b.startswith(needle) for b in bad), (name, mistake, bad)


@pytest.mark.parametrize("iteration", PG.ITERATIONS)
def test_the_comparison_rejects_zero_decay_as_a_product_with_theta(iteration):
    for name, asg in (("A", "cycle"), ("A", "shifted"), ("C", "cycle"), ("D", "shifted")):
        exp = PG.expected(name, asg, iteration, "inf_theta")
        bad = PG.compare(_mutant(name, asg, iteration, "inf_theta", decay_always=True), exp)
        assert any(b.startswith("theta") for b in bad), (name, asg, bad)
        assert PG.compare(_mutant(name, asg, iteration, "plain", decay_always=True), PG.expected(name, asg, iteration)) == []      # only the Inf shows it


def test_the_comparison_rejects_skipped_counted_per_workgroup():
    for name in ("A", "C", "D"):
        exp = PG.expected(name, "cycle", 5, "nonfinite_skip")
        bad = PG.compare(_mutant(name, "cycle", 5, "nonfinite_skip", skipped_per_workgroup=True), exp)
        assert bad and all(b.startswith("rec.skipped") for b in bad), bad
    exp = PG.expected("A", "cycle", 5, "nonfinite_skip")
    assert PG.compare(dict(exp, rec=None), exp) != [] and PG.compare(dict(exp, rec=(np.nextafter(np.float32(PG.COEF), np.float32(1)), 2, 8)), exp) != []
    assert PG.compare(dict(exp, rec=(PG.COEF, 3, 8)), exp) != []


@pytest.mark.parametrize("name,assignment", [("A", "cycle"), ("A", "shifted"), ("D", "cycle"), ("D", "shifted")])
def test_the_mask_comparison_rejects(name, assignment):
    g, seg, rows = PG.mask_gradient(name, assignment), PG.table(name), PG.rows(name, assignment)
    exp = TS.mask_reference(g, seg, rows)
    assert PG.compare_mask(exp, exp) == []
    frozen = [s for s in range(len(rows)) if rows[s]["frozen"]]
    neg = exp.copy()
    for s in frozen:
        neg[seg[s]:seg[s + 1]] = np.float32(-0.0)
    assert PG.compare_mask(neg, exp) != []                                                # -0.0 is not the word 0
    nan = exp.copy()
    keep = np.isnan(g) & (PG.bits(exp) == 0)
    assert keep.any()
    nan[keep] = g[keep]                                                                   # g *= 0 leaves a NaN a NaN
    assert PG.compare_mask(nan, exp) != []
    shifted = np.roll(rows, 1)                                                            # the neighbour's row
    assert PG.compare_mask(TS.mask_reference(g, seg, shifted), exp) != []
    allz = np.zeros_like(exp)
    assert PG.compare_mask(allz, exp) != [] and PG.compare_mask(g, exp) != []
