"""CPU: the comparison of tests/test_stream_gpu.py is sharp.  Each mutant of StreamReference (stream_parity.MUTANTS: a plausible mistake of the
append or the agree kernel) is driven through the scenario of the GPU test that covers it; `mismatches` against the true reference's
snapshots must name a difference, as it would for a kernel that made the mistake."""
import pytest

import stream_parity as P


@pytest.fixture(scope="module")
def truth():
    at, gt = P.append_ticks(), P.agree_ticks()
    return dict(append=(at, {0: P.run_append(P.new_append_reference(), at)}),
                agree=(gt, {A: P.run_agree(P.new_agree_reference(A), gt)[0] for A in (2, 3)}))


def test_the_reference_equals_itself(truth):
    at, want = truth["append"]
    assert not P.mismatches(P.run_append(P.new_append_reference(), at), want[0])
    gt, want = truth["agree"]
    assert not P.mismatches(P.run_agree(P.new_agree_reference(3), gt)[0], want[3])


@pytest.mark.parametrize("name", sorted(P.MUTANTS))
def test_each_mutant_is_rejected(truth, name):
    cls, scenario = P.MUTANTS[name]
    ticks, want = truth[scenario]
    if scenario == "append":
        bad = P.mismatches(P.run_append(P.new_append_reference(cls), ticks), want[0])
        print(f"{name}: {len(bad)} arrays differ, first {bad[:3]}")
        assert bad, f"{name}: the append scenario does not see it"
    else:
        for A in (2, 3):
            bad = P.mismatches(P.run_agree(P.new_agree_reference(A, cls), ticks)[0], want[A])
            print(f"{name} A={A}: {len(bad)} arrays differ, first {bad[:3]}")
            assert bad, f"{name}: the agree scenario does not see it at A={A}"
