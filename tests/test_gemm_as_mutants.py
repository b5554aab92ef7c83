"""CPU: the checks of tests/test_gemm_as_gpu.py have teeth.  Eleven ordinary mistakes are applied to the fp64 reference of tests/gemm_as_parity.py,
not to the kernel (an element the mistaken kernel would never store holds the sentinel, as the guarded output buffer would):
  stale_weights           one workgroup multiplies, at its last column step, the weights its ring slot held one lap earlier (step s - R)
  held_at_odd_columns     the held even-step group is stored at the odd step's columns
  last_odd_step_dropped   under paired stores the last step of an odd step count is never stored
  second_pass_dropped     the second row pass is dropped when the last workgroup has more rows than the first pass takes
  clamp_off_by_one        A rows clamped to M - 2: the last row multiplies its neighbour's
  split_overlap           a column split stages its weight rows from one step below its own
  no_pair_permutation     the pair permutation of 16-bit C left out: columns 4..7 and 8..11 of every 16 exchanged
  pa_neighbour_sample     P / Q taken from the neighbouring sample
  bias_past_n_valid       the bias is read, and the group stored, in the columns >= n_valid
  rowscale_modes_swapped  rowscale_bias 0 and 1 exchanged
  qkv_layouts_swapped     head_major 0 and 1 exchanged
Each must break array_equal in at least one exact case and exceed the real-valued bound by a factor of 2 at least in one case; the margins are
printed (pytest -s).  decode and describe_wrong must name the injected step and row faults on the fingerprint cases."""
import numpy as np
import pytest

import gemm_as_parity as G

SMALL = [c for c in G.CASES if c.M * c.N * c.K < 3e8 and c.pro != "ln"]          # the second pass of the 192-row form has its own, cheapest, cases
BIG_ROWS = ["k512_m32769", "pa_k512_rows192"]


def _targets(mut, exact):
    pool = [G.BY_NAME[n] for n in BIG_ROWS] if mut == "second_pass_dropped" else SMALL
    return [c for c in pool if G.mutant_applies(c, mut) and not c.fp and (not exact or not c.real_only)][:4]


def _differ(a, b):
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


@pytest.mark.parametrize("mut", G.MUTANTS)
def test_each_mistake_breaks_an_exact_case(mut):
    hits = {}
    for c in _targets(mut, True):
        op, masks = G.inputs(c.name, False), G.cpu_masks(c)
        ref, wrong = G.reference(c, op, masks), G.reference(c, op, masks, mut=mut)
        hits[c.name] = sum(int(_differ(ref[n], wrong[n]).sum()) for n in ref)
    print(f"gemm_as mutant {mut}: wrong elements in the exact form {hits}")
    assert hits and max(hits.values()) > 0, (mut, hits)


@pytest.mark.parametrize("mut", G.MUTANTS)
def test_each_mistake_exceeds_the_real_valued_bound(mut):
    margins = {}
    for c in _targets(mut, False):
        if c.real_only:
            continue
        op, masks = G.inputs(c.name, True), G.cpu_masks(c)
        ref, bound = G.reference(c, op, masks, rounded=False), G.bounds(c, op, masks)
        assert all(np.isfinite(b).all() and (b >= 0).all() for b in bound.values())
        wrong = G.reference(c, op, masks, mut=mut, rounded=False)
        margins[c.name] = max(G.worst_ratio(c, wrong, ref, bound).values())
    print(f"gemm_as mutant {mut}: worst error / bound " + " ".join(f"{n}={v:.3g}" for n, v in margins.items()))
    assert margins and max(margins.values()) >= 2.0, (mut, margins)


@pytest.mark.parametrize("name", ["fp_step_k256", "fp_step_k512", "fp_lane_k256", "fp_lane_k512"])
def test_decode_and_the_message_name_the_injected_step_and_row_faults(name):
    c = G.BY_NAME[name]
    p = G.plan(name)
    op = G.inputs(name, False)
    ref = G.reference(c, op, {})["C"]
    # a stale ring slot: the last workgroup's last step holds the weights of step s - R
    stale = G.reference(c, op, {}, mut="stale_weights")["C"]
    s, m = p.nsteps - 1, c.M - 1
    if c.fp == "step":
        n = s * 32 + 5
        assert G.decode(c, stale[m, n], m, n)["weights"] == s - p.ring and G.decode(c, ref[m, n], m, n)["weights"] == s
        msg = G.describe_wrong(c, "C", stale, ref)
        m0, n0 = (int(i) for i in np.argwhere(stale != ref)[0])
        assert (m0 // p.rows, n0 // 32) == (p.gx - 1, s)
        assert f"({m0}, {n0}) workgroup ({p.gx - 1}, 0) pass 0" in msg and f"step {s} slot {s % p.ring}" in msg
        assert f"weights of step {s - p.ring} (want {s})" in msg, msg
    else:          # every step stages the same 32 row values: a stale slot cannot show on the lane fingerprint, a shifted staged row does
        assert np.array_equal(stale, ref)
        shifted = ref.copy()
        shifted[m, 32:64] = np.roll(ref[m, 32:64], 1)
        assert G.decode(c, shifted[m, 40], m, 40)["weights"] == 7 and G.decode(c, ref[m, 40], m, 40)["weights"] == 8
        assert "weights of weight row 7 (want 8)" in G.describe_wrong(c, "C", shifted, ref, limit=40)
    # a row fault: the clamp one row short makes the last row multiply its neighbour's activations
    clamped = G.reference(c, op, {}, mut="clamp_off_by_one")["C"]
    a_own, a_nb = int(G.fp_row_factor(c.M - 1)), int(G.fp_row_factor(c.M - 2))
    assert a_own != a_nb
    hits = [n for n in range(c.N) if clamped[m, n] != ref[m, n]]
    assert hits and all(G.decode(c, clamped[m, n], m, n)["a"] == a_nb for n in hits)
    msg = G.describe_wrong(c, "C", clamped, ref)
    L = G.locate(c, m, hits[0])
    assert f"({m}, {hits[0]}) workgroup ({L['x']}, 0) pass 0 wave {L['wave']} row tile {L['tile']}" in msg and f"activations a {a_nb} (want {a_own})" in msg, msg


def test_failure_message_names_pass_wave_and_slot_of_the_chunked_kernel():
    c = G.BY_NAME["chunk_k512_last257"]
    op, masks = G.inputs(c.name, False), G.cpu_masks(c)
    ref, wrong = G.reference(c, op, masks), G.reference(c, op, masks, mut="second_pass_dropped")
    msg = G.describe_wrong(c, "C", wrong["C"], ref["C"])
    m = 128 * 384 + 256                              # the one row of the second pass
    assert f"({m}, 0) workgroup (128, 0) pass 1 wave 0 row tile 0 step 0 slot 0 sub 0" in msg and "1 x 0..191" not in msg, msg
    assert int((wrong["C"] != ref["C"]).sum()) == c.N
