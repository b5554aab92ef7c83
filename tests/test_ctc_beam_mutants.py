"""CPU: the rows of ctc_beam_parity.py reject ordinary mistakes of a beam-search kernel.  Each mistake of ctc_beam_parity.MUTANTS is switched
on in the fp64 tracer on the rows it is looked for on; on at least one of them the expected n-best list of a kept clip must change (other
symbols, another length, or a score further off than the row's tau / 2, the bound of the GPU test) -- a kernel making that mistake cannot
pass tests/test_ctc_beam_edges_gpu.py.  The test prints the rows and the number of clips that change."""
import pytest

import ctc_beam_parity as P

BY_ID = {P.case_id(c): c for c in P.CASES + P.TIE_CASES}
EX_ROWS = [P.case_id(c) for c in P.CASES if c.ex]
# mistake -> the rows it is looked for on
MUTANT_ROWS = {
    # a stale-parent merge (the child's recorded parent node is not the parent's current node) treated as no merge: a duplicate prefix
    "stale_no_merge": ["W5-T33-C3-blank1-nb5-nolm-s3", "W16-T33-C3-blank2-nb16-aut3-s3", "W32-T33-C3-blank2-nb32-nolm-s3"],
    # a merge accepted wherever the lengths fit and the last classes agree, the chains unseen (an equal hash or parent id taken as identity)
    "loose_merge": ["W3-T16-C3-blank0-nb3-aut3-s3", "W17-T17-C5-blank4-nb1-nolm-s3", "W32-T33-C60-blank59-nb32-nolm"],
    "merged_tot_for_pb": ["W4-T15-C2-blank0-nb2-nolm-s3", "W8-T16-C2-blank1-nb8-aut3-s3", "W24-T15-C3-blank2-nb12-tab-s3"],
    "tie_order": [P.case_id(c) for c in P.TIE_CASES],
    "wave_first_beam_only": ["W17-T15-C33-blank16-nb17-nolm", "W24-T16-C64-blank63-nb24-nolm", "W32-T17-C64-blank63-nb16-aut3-ex"],
    "wave_top16": ["W17-T1-C64-blank32-nb17-tab", "W24-T1-C33-blank32-nb24-nolm", "W31-T17-C33-blank32-nb16-nolm-conf", "W32-T1-C64-blank0-nb32-nolm"],
    "chunk_first_skipped": ["W1-T5-C2-blank1-nb1-nolm-s3", "W2-T9-C64-blank0-nb2-nolm-conf", "W3-T17-C60-blank30-nb1-nolm", "W32-T33-C60-blank59-nb32-nolm"],
    "chunk_first_twice": ["W1-T5-C2-blank1-nb1-nolm-s3", "W2-T9-C64-blank0-nb2-nolm-conf", "W3-T17-C60-blank30-nb1-nolm", "W32-T33-C60-blank59-nb32-nolm"],
    "tail_dropped": ["W1-T5-C2-blank1-nb1-nolm-s3", "W2-T9-C64-blank0-nb2-nolm-conf", "W8-T15-C64-blank63-nb8-nolm", "W16-T17-C33-blank32-nb16-tab"],
    "lane32_dropped": ["W1-T4-C64-blank32-nb1-aut3", "W4-T17-C33-blank16-nb4-tab-conf", "W15-T16-C33-blank0-nb1-nolm", "W32-T1-C64-blank0-nb32-nolm"],
    "blank_last": ["W2-T1-C2-blank0-nb2-nolm-s3", "W3-T17-C60-blank30-nb1-nolm", "W32-T15-C60-blank30-nb32-aut3"],
    "last_frame_ignored": ["W1-T1-C60-blank59-nb1-nolm", "W5-T16-C64-blank32-nb3-tab", "W32-T16-C33-blank32-nb32-tab"],
    "eos_dropped": ["W1-T3-C3-blank0-nb1-tab-s3", "W4-T1-C64-blank63-nb4-aut3", "W32-T17-C64-blank63-nb16-aut3-ex"],
    "rank_before_eos": ["W8-T1-C33-blank0-nb4-tab", "W17-T1-C64-blank32-nb17-tab", "W32-T16-C33-blank32-nb32-tab"],
    "nbest_beam_order": ["W8-T1-C33-blank0-nb4-tab", "W17-T1-C64-blank32-nb17-tab", "W32-T16-C33-blank32-nb32-tab"],
    "len_is_T": EX_ROWS,
}
assert set(MUTANT_ROWS) == set(P.MUTANTS)


def _changed(bt, mut):
    return sum(P.first_difference(r, g, bt.tau / 2) is not None for r, g in zip(bt.expected, P.expected(bt, mut)))


@pytest.mark.parametrize("mut", P.MUTANTS)
def test_mutant_changes_the_expected_output(mut):
    hits = {}
    for rid in MUTANT_ROWS[mut]:
        n = _changed(P.build(BY_ID[rid]), mut)
        if n:
            hits[rid] = n
    print(f"{mut}: clips whose expected n-best changes, per row: {hits}")
    assert hits, f"{mut} changes no row of {MUTANT_ROWS[mut]}"


def test_tie_order_is_invisible_on_every_decidable_row():
    """why the tie rows exist: a margin above tau excludes every tie that the output depends on, so no row of the table sees the tie order"""
    for rid in ("W5-T33-C3-blank1-nb5-nolm-s3", "W32-T33-C60-blank59-nb32-nolm", "W17-T1-C64-blank32-nb17-tab"):
        assert _changed(P.build(BY_ID[rid]), "tie_order") == 0


def test_no_mistake_is_no_change():
    for rid in ("W17-T33-C3-blank0-nb17-tab-ex-s3", "W32-T2-C64-blank63-nb32-nolm-twin"):
        assert _changed(P.build(BY_ID[rid]), None) == 0
