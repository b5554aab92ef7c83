"""CPU: the case table of ctc_beam_parity.py is what tests/test_ctc_beam_edges_gpu.py needs it to be.  The tracer is prefix_beam_search on
every clip of every row; every kept clip is decidable (margin above the row's derived tau) and every row accepts at least a quarter of its
draws; and the table as a whole reaches the kernel's edges, counted by the tracer: stale-parent merges, the second beam of a wave, frames
with fewer / exactly / more than W candidates, a wave without a beam, a merged same-prefix survivor, a last frame that changes the top
hypothesis, a final ranking the end-of-string LM term reorders, and ragged clips that end on and one past a chunk boundary."""
import numpy as np
import pytest

import ctc_beam_parity as P
from ishara_amd.ctc_beam import check_device_args, prefix_beam_search

ALL = P.CASES + P.TIE_CASES


def _total(bt, key):
    return sum(c[key] for c in bt.counters)


def test_the_table_has_the_dimensions_it_promises():
    assert 55 <= len(P.CASES) <= 65
    ids = [P.case_id(c) for c in ALL]
    assert len(set(ids)) == len(ids)

    def twice(values, got):
        for v in values:
            assert sum(g == v for g in got) >= 2, (v, got)
    twice([1, 2, 3, 4, 5, 8, 15, 16, 17, 24, 31, 32], [c.W for c in P.CASES])
    twice([2, 3, 5, 33, 60, 64], [c.C for c in P.CASES])
    twice(["none", "table", "aut3"], [c.lm for c in P.CASES])
    twice(["last", "first", "mid"], ["last" if c.blank == c.C - 1 else "first" if c.blank == 0 else "mid" for c in P.CASES])
    twice(["one", "all", "between"], ["between" if 1 < c.nbest < c.W else "one" if c.nbest == 1 else "all" for c in P.CASES])
    for W in sorted({c.W for c in P.CASES}):                # every beam width meets every frame-count edge of its own chunk
        ch = P.chunk(W)
        assert {c.T for c in P.CASES if c.W == W} >= {1, ch - 1, ch, ch + 1, 2 * ch + 1}, W
    assert {P.chunk(W) for W in (1, 2, 3, 32)} == {4, 8, 16}
    ex = [c for c in P.CASES if c.ex]
    assert len(ex) >= 4 and {c.lm for c in ex} == {"none", "table", "aut3"}
    for c in ex:
        ch = P.chunk(c.W)
        assert {1, ch, ch + 1, c.T} <= set(P.case_lengths(c).tolist()), P.case_id(c)
    assert all(8 <= c.B <= 16 for c in ALL)
    assert any(c.alpha != 0 and c.beta != 0 and c.lm == "table" for c in P.CASES)


@pytest.mark.parametrize("case", ALL, ids=P.case_id)
def test_tracer_is_the_reference_and_every_clip_is_decidable(case):
    bt = P.build(case)
    check_device_args(case.C, case.T, case.W, case.nbest)
    assert bt.x.shape == (case.B, case.T, case.C) and bt.x.dtype == np.float32
    assert P.TAU_MIN <= bt.tau <= P.TAU_MAX and (bt.tau == P.TAU_MIN or bt.tau == P.TAU_MAX or bt.tau == P.TAU_FACTOR * bt.E)
    assert bt.share >= 0.25, bt.share
    for b in range(case.B):
        n = int(bt.lens[b])
        assert bt.margins[b] > bt.tau, (b, bt.margins[b], bt.tau)
        assert bt.E_clip[b] <= bt.E
        plain = P.trace(bt.x[b, :n], case.W, case.nbest, bt.lm, case.alpha, case.beta, case.blank)
        ref, margin = prefix_beam_search(bt.x[b, :n], case.W, case.nbest, lm=bt.lm, alpha=case.alpha, beta=case.beta, blank=case.blank,
                                         return_margin=True)
        full = prefix_beam_search(bt.x[b, :n], case.W, case.W, lm=bt.lm, alpha=case.alpha, beta=case.beta, blank=case.blank, return_margin=True)[1]
        assert [h[0].tolist() for h in plain.hyps] == [r[0].tolist() for r in ref], b
        np.testing.assert_allclose([h[1] for h in plain.hyps], [r[1] for r in ref], rtol=1e-12, atol=0)
        assert plain.margin == margin and plain.margin_full == full
        if case.kind != "twin":                             # the expected lists are the plain tracer's; a tie row's rank the tie classes
            assert P.first_difference(plain.hyps, bt.expected[b], 0.0) is None
            assert bt.margins[b] == full
        else:                                               # the same scores; the order inside a tie class is the tie rule's
            np.testing.assert_allclose(sorted(h[1] for h in plain.hyps), sorted(h[1] for h in bt.expected[b]), rtol=1e-12, atol=P.TIE_EPS)


def test_tie_rows_hold_exact_ties_at_the_selection_boundary():
    """what the tie rows are for: without the tie classes the reference's own margin is (numerically) zero on them"""
    hit = 0
    for case in P.TIE_CASES:
        bt = P.build(case)
        for b in range(case.B):
            m = prefix_beam_search(bt.x[b], case.W, case.W, blank=case.blank, return_margin=True)[1]
            hit += int(m <= P.TIE_EPS)
            assert bt.margins[b] > bt.tau
    assert hit >= len(P.TIE_CASES)


def test_the_table_reaches_the_kernels_edges():
    built = [P.build(c) for c in P.CASES]
    stale = {P.case_id(bt.case): _total(bt, "stale") for bt in built}
    print("stale-parent merges per row:", {k: v for k, v in stale.items() if v})
    assert sum(stale.values()) >= 20
    assert any(v > 0 and bt.case.W <= 16 for bt, v in zip(built, stale.values()))
    assert any(v > 0 and bt.case.W > 16 for bt, v in zip(built, stale.values()))
    for key in ("second_beam_kept", "frames_nb_lt_W", "frames_cand_eq_W", "frames_cand_gt_W", "merged_same_kept", "last_frame_changes_top",
                "eos_reorders"):
        rows = [P.case_id(bt.case) for bt in built if _total(bt, key) > 0]
        print(key, len(rows), "rows")
        assert rows, key
    assert any(_total(bt, "second_beam_kept") for bt in built if 16 < bt.case.W < 32)        # a wave with two beams beside waves with one
    assert any(P.waves(c.W) > c.W for c in P.CASES)                                           # a wave without a beam
    ex = [bt for bt in built if bt.case.ex]
    assert any(c["ends_on_chunk"] for bt in ex for c in bt.counters)
    assert any(c["ends_past_chunk"] for bt in ex for c in bt.counters)
    assert any(len(c["chunks"]) >= 3 for bt in built for c in bt.counters)                    # a clip that crosses two chunk boundaries
