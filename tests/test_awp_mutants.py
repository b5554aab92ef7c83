"""CPU: the comparison tests/test_awp_gpu.py applies to the kernel (awp_parity.compare) accepts the reference and rejects ordinary mistakes,
each restated in numpy on the parity vectors: an FMA in w + scale * g, one global norm, a dropped eps, the sum of squares where its root
belongs, a segment boundary off by one, a step down the gradient, an fp32 sum of the squares, a perturbed NaN segment."""
import math

import numpy as np
import pytest

import awp_parity as AP


def _mutant(name, variant="plain", relative=False, *, fma=False, global_norm=False, no_eps=False, no_sqrt=False, shift=0, sign=1.0,
            f32_sum=False, perturb_nonfinite=False):
    """ishara_awp_perturb with the chosen mistakes -> a result as awp_parity.compare takes it"""
    w, g = AP.vectors(name, variant)
    seg = [int(o) for o in AP.table(name)]
    if shift:
        seg = [seg[0]] + [o + shift for o in seg[1:-1]] + [seg[-1]]
    delta, eps = float(np.float32(AP.DELTA)), 0.0 if no_eps else float(np.float32(AP.EPS))
    out, scale = w.copy(), np.zeros(len(seg) - 1, np.float32)
    tot_g = tot_d = 0.0
    zeroed = 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        all_ss = float(np.sum(g.astype(np.float64) ** 2))
        for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
            gs, ws = g[lo:hi], w[lo:hi]
            ss = float(np.sum(gs * gs, dtype=np.float32)) if f32_sum else float(np.sum(gs.astype(np.float64) ** 2))
            ssw = float(np.sum(ws.astype(np.float64) ** 2))
            if global_norm:
                ss = all_ss
            if not (math.isfinite(ss) and (not relative or math.isfinite(ssw))) and not perturb_nonfinite:
                zeroed += 1
                continue
            root = ss if no_sqrt else math.sqrt(ss) if ss >= 0 else float("nan")
            den = root + eps
            num = delta * math.sqrt(ssw) if relative else delta
            scale[s] = np.float32(num / den) if den != 0 else np.float32(np.inf)
            if fma:
                out[lo:hi] = (ws.astype(np.float64) + sign * float(scale[s]) * gs.astype(np.float64)).astype(np.float32)
            else:
                out[lo:hi] = ws + np.float32(sign) * (scale[s] * gs)
            tot_g += ss
            tot_d += float(scale[s]) ** 2 * ss
        stats = dict(grad_norm=float(np.float32(math.sqrt(tot_g))) if tot_g >= 0 else float("nan"),
                     delta_norm=float(np.float32(math.sqrt(tot_d))) if tot_d >= 0 else float("nan"), perturbed=len(scale) - zeroed, zeroed=zeroed)
    return dict(w_adv=out, backup=w.copy(), g_after=g.copy(), scale=scale, stats=stats)


CASES = [(n, v, r) for n in ("A", "B", "C", "D") for v in AP.VARIANTS for r in (False, True)]


@pytest.mark.parametrize("name,variant,relative", CASES)
def test_the_comparison_accepts_the_reference_and_a_faithful_restatement(name, variant, relative):
    ref = AP.reference(name, variant, relative)
    assert AP.compare(ref, name, variant, relative) == []
    assert AP.compare(_mutant(name, variant, relative), name, variant, relative) == []       # np.sum in fp64 instead of math.fsum: inside the ulp
    assert AP.subnormal_intermediates(name, variant, relative) == 0


@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("mistake,needle", [
    (dict(fma=True), "w_adv"),
    (dict(global_norm=True), "scale"),
    (dict(no_eps=True), "scale"),
    (dict(no_sqrt=True), "scale"),
    (dict(shift=1), "scale"),
    (dict(shift=-1), "scale"),
    (dict(sign=-1.0), "w_adv"),
])
def test_the_comparison_rejects(mistake, needle, relative):
    for name in ("A", "C"):
        bad = AP.compare(_mutant(name, "plain", relative, **mistake), name, "plain", relative)
        assert any(b.startswith(needle) for b in bad), (name, mistake, bad)


def test_the_comparison_rejects_a_dropped_eps_on_a_zero_gradient():
    bad = AP.compare(_mutant("A", "zero_grad", no_eps=True), "A", "zero_grad")
    assert any(b.startswith("scale") for b in bad), bad


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_the_comparison_rejects_an_fp32_sum_of_squares(name):
    """on the 3e19 vector the fp32 squares are Inf: the segment is zeroed (or its scale is 0) where the reference perturbs it"""
    assert AP.compare(_mutant(name, "huge", f32_sum=True), name, "huge") != []
    bad = AP.compare(_mutant(name, "huge", f32_sum=True), name, "huge")
    assert any(b.startswith(("scale", "zeroed", "perturbed")) for b in bad), bad
    assert AP.compare(_mutant(name, "huge"), name, "huge") == []


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_the_comparison_rejects_a_perturbed_nan_segment(name):
    bad = AP.compare(_mutant(name, "nonfinite", perturb_nonfinite=True), name, "nonfinite")
    assert any(b.startswith("w_adv") for b in bad) and any(b.startswith(("zeroed", "perturbed")) for b in bad), bad


def test_the_comparison_rejects_a_touched_backup_gradient_or_count():
    ref = AP.reference("A")
    for key in ("backup", "g_after"):
        x = ref[key].copy()
        x[len(x) // 2] = np.nextafter(x[len(x) // 2], np.float32(9))
        assert any(b.startswith(key) for b in AP.compare(dict(ref, **{key: x}), "A"))
    assert AP.compare(dict(ref, stats=dict(ref["stats"], zeroed=1)), "A") != []
    assert AP.compare(dict(ref, stats=dict(ref["stats"], delta_norm=ref["stats"]["delta_norm"] * (1 + 3e-6))), "A") != []
    two = ref["scale"].copy()
    two[3] = np.nextafter(np.nextafter(two[3], np.float32(9)), np.float32(9))
    w, g = AP.vectors("A")
    moved = dict(ref, scale=two, w_adv=AP.recompute(w, g, AP.table("A"), two, np.zeros(len(two), bool)))
    assert any(b.startswith("scale") for b in AP.compare(moved, "A"))              # 2 ulps off, even with w_adv consistent with it
