"""On the cases of tests/test_augment_ex_gpu.py: each ordinary mistake of the spatial affine, the temporal mask or the frame count moves
the host composition past the GPU test's tolerance (rtol 1e-7, atol 1e-6) on some case, in both layouts, by at least 2x: a kernel that
made it could not pass.  The z-normalisation cancels a scale and a shift of a clip without an exactly-zero entry (to ~5e-7, under the
tolerance), so those two mistakes show only on cases with zero frames (padding, a drawn shift, dropout, a mask); a mask edge shows only
where the edge frame is sampled, so the mask cases sit on padded clips (L2 <= T)."""
import numpy as np
import pytest

import augment_ex_parity as AP
from ishara_amd import data as D

MUTANTS = ["M_transposed", "shift_on_z", "scale_dropped", "shift_dropped", "affine_after_mirror", "shift_on_zero_frames",
           "mask_one_short", "mask_one_late"]


def _excess(bad, ref):
    """max over the values of |bad - ref| / (atol + rtol |ref|): > 1 fails assert_allclose"""
    return float((np.abs(bad.astype(np.float64) - ref) / (AP.TOL["atol"] + AP.TOL["rtol"] * np.abs(ref))).max())


@pytest.mark.parametrize("mut", MUTANTS)
def test_tolerance_rejects_the_mistake(mut):
    clips, cases = AP.clips(), AP.cases()
    T = 64
    ref = AP.reference(T)
    worst = {layout: 0.0 for layout in AP.LAYOUTS}
    killers = 0
    for i, (ci, d) in enumerate(cases):
        if mut.startswith("mask") and d.m1 == d.m0:
            continue
        if not mut.startswith("mask") and d.M == (1.0, 0.0, 0.0, 1.0):
            continue
        bad = AP.host(clips[ci][0], d, T, mut)
        ex = {layout: _excess(D.to_features(bad, layout), D.to_features(ref[i], layout)) for layout in AP.LAYOUTS}
        killers += min(ex.values()) >= 2.0
        for layout in AP.LAYOUTS:
            worst[layout] = max(worst[layout], ex[layout])
    print(mut, {k: f"{v:.3g}x" for k, v in worst.items()}, f"{killers} cases reject it in both layouts")
    if mut == "shift_on_z":                                 # hands_lips_xy carries no z: the flat cases reject it
        assert worst["flat"] >= 2.0
    else:
        assert killers >= 1 and min(worst.values()) >= 2.0


def test_scale_and_shift_need_zero_frames():
    """the case-selection fact: without an exactly-zero entry the normalisation cancels a dropped scale or shift under the tolerance"""
    clips, cases = AP.clips(), AP.cases()
    T = 32
    ref = AP.reference(T)
    full = [(i, ci, d) for i, (ci, d) in enumerate(cases)
            if d.draw.n == 385 and d.draw.shift is None and not d.draw.windows and d.m0 == d.m1 and d.M != (1.0, 0.0, 0.0, 1.0) and d.draw.L2 > T]
    assert full
    for i, ci, d in full:
        for mut in ("scale_dropped", "shift_dropped"):
            assert _excess(AP.host(clips[ci][0], d, T, mut), ref[i]) < 1.0, (mut, d)


def test_frame_len_mistake_is_visible():
    """frame_len = L2 instead of min(L2, T) differs on the cases with L2 > T; L2 instead of 0 on an empty clip is not reachable from
    the draws (n == 0 gives L2 == 0) and is pinned by a forced row in the GPU test"""
    for T in AP.TS:
        assert any(d.draw.L2 > T and AP.frame_len(d, T) == T for _, d in AP.cases())
        assert any(0 < d.draw.L2 < T for _, d in AP.cases())
    assert any(d.draw.L2 == 0 and d.draw.n > 0 for _, d in AP.cases())
