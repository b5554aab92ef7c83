"""CPU: the checks of tests/test_gemm_nt_gpu.py have teeth.  Ten ordinary mistakes are applied to the fp64 reference of tests/gemm_nt_parity.py:
  drop_last_ktile           the last K tile is never multiplied
  stale_slot                one output tile multiplies, at its last K tile, what the ring slot held one lap earlier (kt - 3 / kt - 4)
  clamp_off_by_one          A rows clamped to M - 2: the last row multiplies its neighbour's
  bias_guard_tile           the bias guard tests the column tile, not the column: a ragged last column tile gets no bias
  resid_neighbour_group     one 16-row group takes the residual of the next one
  second_tile_first_coords  a persistent workgroup's second tile is computed at its first tile's (mt, nt)
  rowscale_modes_swapped    rowscale_bias 0 and 1 exchanged
  dact_after_resid          the residual is added before act' is applied
  qkv_layouts_swapped       head_major 0 and 1 exchanged
  vt_not_transposed         V written [B, H, T, dh] into vt
Each must break array_equal in at least one exact case and exceed the real-valued bound in at least one case; the margins are printed (pytest -s).
decode must name the injected K-tile faults on the fingerprint cases."""
import numpy as np
import pytest

import gemm_nt_parity as G

SMALL = [c for c in G.RUN_CASES if c.M * c.N * c.K < 2e8]          # the persistent mutant has its own, cheapest, persistent case
PERSISTENT = "t_p769_row1"


def _targets(mut, exact):
    pool = [G.BY_NAME[PERSISTENT]] if mut == "second_tile_first_coords" else SMALL
    return [c for c in pool if G.mutant_applies(c, mut) and not c.fp and (not exact or not c.real_only)][:4]


@pytest.mark.parametrize("mut", G.MUTANTS)
def test_each_mistake_breaks_an_exact_case(mut):
    hits = {}
    for c in _targets(mut, True):
        op, masks = G.inputs(c.name, False), G.cpu_masks(c)
        ref, wrong = G.reference(c, op, masks), G.reference(c, op, masks, mut=mut)
        hits[c.name] = sum(int((ref[n] != wrong[n]).sum()) for n in ref)
    print(f"gemm_nt mutant {mut}: wrong elements in the exact form {hits}")
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
    print(f"gemm_nt mutant {mut}: worst error / bound " + " ".join(f"{n}={v:.3g}" for n, v in margins.items()))
    assert margins and max(margins.values()) >= 2.0, (mut, margins)


@pytest.mark.parametrize("name", ["t_fpW", "t_fpA", "g_fpW", "g_fpA"])
def test_decode_names_the_injected_k_tile_faults(name):
    c = G.BY_NAME[name]
    op, n = G.inputs(name, False), G.nk(c)
    ref = G.reference(c, op, {})["C"]
    m = c.M - 1
    a = 1 if c.fp == "W" else int(G.fp_row_factor(m))
    assert G.decode(ref[m, 0], n) == [a] * n
    dropped = G.reference(c, op, {}, mut="drop_last_ktile")["C"]
    assert G.decode(dropped[m, 0], n) == [a] * (n - 1) + [0]
    stale = G.reference(c, op, {}, mut="stale_slot")["C"]          # the last tile's last K tile holds the digit of kt - ring: that digit twice, kt's missing
    want = [a] * n
    want[n - 1], want[n - 1 - G.ring(c)] = 0, 2 * a
    assert G.decode(stale[m, c.N - 1], n) == want
    msg = G.describe_wrong(c, "C", stale, ref)
    m0 = int(np.argwhere(stale != ref)[0][0])                        # the message lists the first wrong elements: that row's digits
    a0 = 1 if c.fp == "W" else int(G.fp_row_factor(m0))
    want0 = [a0] * n
    want0[n - 1], want0[n - 1 - G.ring(c)] = 0, 2 * a0
    assert f"digits got {want0} want {[a0] * n}" in msg and "tile (" in msg and (("workgroup" in msg and "round 0" in msg) == (c.route == "NT_TILE_T"))
    doubled = 2 * ref - dropped                                        # the last K tile twice
    assert G.decode(doubled[m, 0], n) == [a] * (n - 1) + [2 * a]


def test_failure_message_names_tile_workgroup_and_round():
    c = G.BY_NAME[PERSISTENT]
    op, masks = G.inputs(c.name, False), G.cpu_masks(c)
    ref, wrong = G.reference(c, op, masks), G.reference(c, op, masks, mut="second_tile_first_coords")
    msg = G.describe_wrong(c, "C", wrong["C"], ref["C"])
    assert "tile (768, 0) id 768 workgroup 0 round 1" in msg, msg
