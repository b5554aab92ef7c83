"""CPU: the host side of the rescoring sweep (ishara_amd/rescore.py): rescore_sweep_reference against brute force, sweep_grid's order and
dtype, sweep_scores against evaluation.mean_score, the coverage condition of tests/rescore_sweep_parity.py and the refusals of the Python
layer.  The device is held to the same reference in tests/test_rescore_sweep_gpu.py."""
import itertools

import numpy as np
import pytest

import rescore_sweep_parity as SP
from ishara_amd import evaluation, mbr, rescore
from ishara_amd.tflite_batch import apply_fallback

CASES = {c["name"]: c for c in SP.cases()}


@pytest.mark.parametrize("fallback", [0, 1])
def test_reference_equals_brute_force_on_the_C3_case(fallback):
    """every row through rescore_reference + levenshtein, written out here"""
    case = CASES["C3"]
    lists = mbr.nbest_to_lists(case["hyp_idx"], case["hyp_len"])
    ref = SP.reference("C3", fallback)
    M = case["M"]
    for b in range(case["B"]):
        tgt = [int(v) for v in case["targets"][b] if v != SP.PAD]
        for g, row in enumerate(case["grid"]):
            order, _, live, _ = rescore.rescore_reference(lists[b], case["logps"][:, b], row[:M], case["lm"], row[M], row[M + 1], 1.0, case["blank"])
            h = np.asarray(lists[b][order[0]] if live[0] else [], np.int64)
            h = apply_fallback(h) if fallback else h
            assert ref["best"][g, b] == (order[0] if live[0] else -1)
            assert ref["dist"][g, b] == evaluation.levenshtein(h.tolist(), tgt)
        assert ref["tlen"][b] == len(tgt)
    assert (ref["best"] >= 0).any()


def test_sweep_grid_order_and_dtype():
    grid = rescore.sweep_grid([[1.0, 0.5], [0.0, 2.0, 3.0]], [0.1, 0.2], [0.0, -1.0, 1.0, 4.0])
    assert grid.dtype == np.float32 and grid.shape == (2 * 3 * 2 * 4, 4)
    want = np.array(list(itertools.product([1.0, 0.5], [0.0, 2.0, 3.0], [0.1, 0.2], [0.0, -1.0, 1.0, 4.0])), np.float32)
    assert np.array_equal(grid, want)
    assert np.array_equal(grid[:5, 3], np.float32([0.0, -1.0, 1.0, 4.0, 0.0])) and (grid[:12, 0] == 1.0).all()      # beta fastest, w_0 slowest
    one = rescore.sweep_grid([[1.0]], 0.5, [0.25])
    assert one.shape == (1, 3) and np.array_equal(one[0], np.float32([1.0, 0.5, 0.25]))
    with pytest.raises(ValueError):
        rescore.sweep_grid([], [0.0], [0.0])
    with pytest.raises(ValueError):
        rescore.sweep_grid([[1.0], []], [0.0], [0.0])
    with pytest.raises(ValueError):
        rescore.sweep_grid([[1.0]] * 9, [0.0], [0.0])
    with pytest.raises(ValueError):
        rescore.sweep_grid([list(range(300))], list(range(300)), [0.0])


def test_sweep_scores_equals_mean_score():
    g = np.random.default_rng(11)
    chars = "abcdefg"
    targets = ["".join(g.choice(list(chars), int(g.integers(1, 9)))) for _ in range(6)]
    preds = [["".join(g.choice(list(chars), int(g.integers(0, 9)))) for _ in range(6)] for _ in range(5)]
    preds.append(list(preds[1]))                             # rows 1 and 5 have equal means: grid order decides
    dist = np.array([[evaluation.levenshtein(p, t) for p, t in zip(row, targets)] for row in preds])
    tlen = np.array([len(t) for t in targets])
    means, ranking = rescore.sweep_scores(dist, tlen)
    assert means.dtype == np.float64 and all(means[r] == evaluation.mean_score(row, targets) for r, row in enumerate(preds))
    assert sorted(ranking.tolist()) == list(range(6)) and (np.diff(means[ranking]) <= 0).all()
    assert ranking.tolist().index(1) < ranking.tolist().index(5)
    with pytest.raises(ValueError):
        rescore.sweep_scores(dist, tlen[:-1])


def test_the_cases_are_not_vacuous():
    """by the reference alone: in the random cases at least half of the clips have three or more distinct winners across the grid, and in
    every case with more than one slot some row picks a slot other than 0"""
    random = [c for c in SP.cases() if c["coverage"]]
    assert len(random) >= 5
    for case in SP.cases():
        many, other = SP.coverage(case)
        print(f"{case['name']}: {many:.2f} of the clips have >= 3 winners; a slot other than 0 wins: {other}")
        if case["coverage"]:
            assert many >= 0.5, case["name"]
        if case["N"] > 1:
            assert other, case["name"]


def test_fallback_changes_the_short_hypotheses_only():
    a, b = SP.reference("lengths", 0), SP.reference("lengths", 1)
    case = CASES["lengths"]
    short = (case["hyp_len"] >= 0) & (case["hyp_len"] < 3)
    assert np.array_equal(a["best"], b["best"]) and np.array_equal(a["hyp_dist"][~short], b["hyp_dist"][~short])
    assert (a["hyp_dist"][short] != b["hyp_dist"][short]).any()
    # the 64-symbol target against its 64- and 70-symbol hypotheses: one substitution, six insertions
    assert a["hyp_dist"][0, 0] == 1 and a["hyp_dist"][0, 1] == 6 and a["tlen"].tolist() == [64, 1, 10]


def test_python_layer_refusals():
    case = CASES["C3"]
    lists = mbr.nbest_to_lists(case["hyp_idx"], case["hyp_len"])
    with pytest.raises(ValueError):
        rescore.rescore_sweep_reference(lists[0], case["logps"][:, 0], case["targets"][0], case["grid"][:, :3])      # M + 1 columns
    with pytest.raises(ValueError):
        rescore.rescore_sweep(case["hyp_idx"], case["hyp_len"], case["logps"][0], case["targets"], case["grid"])     # host arrays: no CPU path
    with pytest.raises(ValueError):
        rescore.rescore_nbest(case["hyp_idx"], case["hyp_len"], case["logps"][0], params=np.zeros(3, np.float32))
