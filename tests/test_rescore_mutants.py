"""CPU: the checks of tests/rescore_parity.py have teeth.  The numpy restatements of ishara_ctc_score_nbest and ishara_nbest_rescore pass every
case; each of the mistakes an alpha recursion, a dedupe, a score sum or a sort invites is rejected by at least one case."""
import numpy as np
import pytest

import rescore_parity as P


def _all_score_cases():
    bad, removed, _ = P.bad_slot_case()
    return list(P.score_cases()) + [bad, removed]


def _ref(case):
    return P.score_reference_of(case) if case["name"].startswith("bad-slots") else P.score_reference(case["name"])


def test_the_restated_score_passes():
    worst = 0.0
    for c in _all_score_cases():
        logp, st = P.restate_score(c)
        fails, ratio = P.check_score(c, logp, st, _ref(c))
        assert not fails, fails[:3]
        worst = max(worst, ratio)
    print(f"fp64 restatement: worst logp err / bound {worst:.3g}")
    bad, removed, want = P.bad_slot_case()
    assert np.array_equal(P.expected_status(bad), want) and set(want.ravel().tolist()) == {0, 1, 2, 4, 8}
    a, b = P.restate_score(bad)[0], P.restate_score(removed)[0]
    assert np.array_equal(a[want == 0], b[want == 0])


@pytest.mark.parametrize("mutant", P.SCORE_MUTANTS)
def test_score_mutant_is_rejected(mutant):
    rejected = {}
    for c in _all_score_cases():
        logp, st = P.restate_score(c, mutant)
        fails, ratio = P.check_score(c, logp, st, _ref(c))
        if fails:
            rejected[c["name"]] = (fails[0][:120], ratio)
    print(f"{mutant}: rejected by {len(rejected)} of {len(_all_score_cases())} cases, e.g. {next(iter(rejected.items()), None)}")
    assert rejected, f"no case rejects {mutant}"


def test_the_rescore_twin_passes():
    worst = 0.0
    for c in P.rescore_cases():
        lp = P.host_logps(c)
        fails, ratio = P.check_rescore(c, P.twin_rescore(c, lp), lp)
        assert not fails, (c["name"], fails[:3])
        worst = max(worst, ratio)
    print(f"float32 twin: worst posterior err / bound {worst:.3f}")


@pytest.mark.parametrize("mutant", P.RESCORE_MUTANTS)
def test_rescore_mutant_is_rejected(mutant):
    rejected = {}
    for c in P.rescore_cases():
        lp = P.host_logps(c)
        fails, ratio = P.check_rescore(c, P.twin_rescore(c, lp, mutant), lp)
        if fails:
            rejected[c["name"]] = fails[0][:120]
    print(f"{mutant}: rejected by {len(rejected)} of {len(P.rescore_cases())} cases, e.g. {next(iter(rejected.items()), None)}")
    assert rejected, f"no case rejects {mutant}"


def test_a_posterior_ten_bounds_off_is_rejected():
    c = next(c for c in P.rescore_cases() if c["name"] == "M3-weights-beta")
    lp = P.host_logps(c)
    base = P.twin_rescore(c, lp)
    assert not P.check_rescore(c, base, lp)[0]
    got = {k: v.copy() for k, v in base.items()}
    got["posterior"][0, 1] *= np.float32(1.0 + 400 * P.EPS * 10)      # the bound at |x| <= 60, n <= 64 is below 400 * 2^-24 relative
    assert P.check_rescore(c, got, lp)[0]
