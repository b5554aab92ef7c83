"""CPU: the real-valued bound of tests/test_gemm_tn_gpu.py has teeth.  The bound is the worst case of fp32 summation (c * M * 2^-24 * the sum
of magnitudes), orders of magnitude above what a correct kernel leaves; this file shows it is still far below what an ordinary mistake leaves.

Three mistakes are applied to the fp64 reference on the real-valued inputs of three cases, and each must exceed the bound by 2x or more on
some output element:
  drop_stage       the last 32-row stage of one M-split is never multiplied (the split comes from the launcher's own plan)
  neighbour_scale  one sample's bias row scale is taken from its neighbour
  no_q             one sample's Q term is left out of the per-sample fold
The cases are the per-sample-affine cases with a bias row scale — the only ones all three mistakes apply to — with the two smallest and the
largest M of the table: the bound grows with M^2 and the trace of a mistake in one stage or one sample does not grow with M, so the largest M is where
the bound is weakest.
The exact form needs no such check: any of these mistakes changes an integer."""
import numpy as np
import pytest

import gemm_tn_parity as G

MUTANTS = ["drop_stage", "neighbour_scale", "no_q"]
APPLICABLE = sorted((c for c in G.RUN_CASES if c.psa_T and c.psa_rs and c.bias), key=lambda c: c.M)
TARGETS = [APPLICABLE[0], APPLICABLE[1], APPLICABLE[-1]]


def test_targets_are_the_two_smallest_and_the_largest():
    assert len(APPLICABLE) >= 3 and len({c.name for c in TARGETS}) == 3
    assert [c.M for c in TARGETS] == [256, 384, 2048]


@pytest.mark.parametrize("mut", MUTANTS)
@pytest.mark.parametrize("name", [c.name for c in TARGETS])
def test_each_mistake_exceeds_the_bound_twice_over(lib, name, mut):
    c = G.BY_NAME[name]
    op = G.inputs(name, True)
    ref, bound = G.reference(c, op), G.bounds(c, op)
    assert all(np.isfinite(b).all() and (b >= 0).all() for b in bound.values())
    wrong = G.reference(c, op, mut=mut, plan=G.plan(lib, c))
    ratio = G.worst_ratio(wrong, ref, bound)
    assert max(ratio.values()) >= 2.0, (name, mut, ratio)
    # and the mistake is one the outputs it does not concern do not see
    untouched = {"neighbour_scale": ("out", "G", "Rpart"), "no_q": ("dbias", "G", "Rpart"), "drop_stage": ()}[mut]
    assert all(ratio[n] == 0.0 for n in untouched), ratio
