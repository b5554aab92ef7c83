"""CPU: the case table of tests/gemm_tn_parity.py contains what it is for.  Route, profiler key, M-splits and rows per split of every case come
from ishara_debug_gemm_tn_plan, i.e. from gemm_tn_plan — the function launch_gemm_tn launches from (host only, nothing is launched).  Every
listed property must hold for the cases that claim it and must have a case; the deferred chains must hold the kinds of call, in the order,
they are for; and the exact form's precondition (every intermediate a multiple of 1/4 below 2^22) holds for every case."""
import numpy as np
import pytest

import gemm_tn_parity as G


@pytest.fixture(scope="module")
def plans(lib):
    return {c.name: G.plan(lib, c) for c in G.CASES}


def test_every_case_has_the_properties_it_is_listed_for(plans):
    wrong = [(c.name, p, plans[c.name]) for c in G.CASES for p in c.props if not G.PROPS[p](c, plans[c.name])]
    assert not wrong, wrong


def test_every_property_has_a_case():
    have = {p for c in G.CASES for p in c.props}
    assert have == set(G.PROPS), (sorted(set(G.PROPS) - have), sorted(have - set(G.PROPS)))


def test_the_plans_the_table_was_chosen_for(plans):
    """(route, splits, rows per split) of the edges, as found when the table was chosen: a change of the split plan moves the table, knowingly"""
    want = {"tr_m2112": ("TN_TR", 8, 288), "tr_m4352": ("TN_TR", 16, 288), "tr_m5184": ("TN_TR", 24, 224), "tr_m4160": ("TN_TR", 130, 32),
            "tr_m7936": ("TN_TR", 248, 32), "tr_24tiles": ("TN_TR", 16, 256), "big": ("TN_BIG", 64, 512), "big_off": ("TN_TR", 32, 1024),
            "psa_b16": ("TN_TR_PSA", 8, 256), "psa_t256_b4": ("TN_TR_PSA", 4, 256), "psa_b7": ("TN_TR_PSA", 1, 896),
            "reg_m299_fa": ("TN_REG", 2, 192), "reg_m299_ff": ("TN_REG", 3, 128)}
    got = {n: (plans[n].route, plans[n].splits, plans[n].rps) for n in want}
    assert got == want


def test_refused_cases_are_refused_with_the_launchers_message(lib, plans):
    for c in G.CASES:
        assert (plans[c.name].route == "TN_REFUSED") == c.refused, c.name
        if c.refused:
            assert plans[c.name] == G.Plan("TN_REFUSED", "", 0, 0)
            G.plan(lib, c)
            msg = lib.ishara_last_error().decode()
            assert msg.startswith("gemm_tn:") and ("per-sample affine" in msg if c.psa_T else "bias row scale" in msg), (c.name, msg)


def test_forced_register_kernel_takes_the_plain_cases(lib):
    assert len(G.FORCED) >= 12
    for c in G.FORCED:
        p = G.plan(lib, c, force=True)
        assert (p.route, p.kernel) == ("TN_REG", "gemm_tn_kernel<bf16,bf16,bf16>") and p.splits >= 1 and p.rps % 64 == 0, (c.name, p)
    # what the switch leaves no kernel for is refused, not run on another one
    for n in ("brs_t96", "psa_b16", "ka_valid_stem", "nb_valid_cls"):
        assert G.plan(lib, G.BY_NAME[n], force=True).route == "TN_REFUSED", n
    assert G.plan(lib, G.BY_NAME["tr_m576"]).route == "TN_TR"          # the switch was restored


def _defers(c, p):
    """a transposed-read call that leaves its sums to the next call (run_tn_tr: tiles * splits <= 256 and splits <= 64)"""
    return p.route in ("TN_TR", "TN_TR_BRS", "TN_TR_PSA") and (p.route == "TN_TR_PSA" or G.tiles(c) * p.splits <= 256) and p.splits <= 64


def test_chains_hold_what_they_are_for(plans):
    ch = [G.BY_NAME[n] for n in G.CHAINS["riders"]]
    pl = [plans[c.name] for c in ch]
    assert len(ch) >= 4 and len({c.name for c in ch}) == len(ch)
    assert _defers(ch[0], pl[0]) and _defers(ch[1], pl[1]) and G.tiles(ch[0]) != G.tiles(ch[1])          # riders carry the first call's sums
    assert pl[2].route == "TN_TR" and pl[2].splits > 64 and G.tiles(ch[2]) * pl[2].splits <= 256          # carries riders, sums at once
    assert pl[3].route == "TN_REG"                                                                          # ignores the deferred state
    assert _defers(ch[4], pl[4]) and pl[4].route == "TN_TR"
    assert pl[5].route == "TN_TR_PSA" and pl[5].splits > 1                                                  # sums call 4's slabs inline, defers its own
    assert _defers(ch[6], pl[6]) and ch[6].nb_valid                                                         # carries the PSA call's sums; padded columns in the riders' job
    assert _defers(ch[7], pl[7]) and pl[7].route == "TN_TR_BRS"                                             # left for the flush
    ch = [G.BY_NAME[n] for n in G.CHAINS["big"]]
    pl = [plans[c.name] for c in ch]
    assert len(ch) >= 4 and _defers(ch[0], pl[0]) and _defers(ch[1], pl[1])
    assert pl[2].route == "TN_BIG"                                                                          # flushes call 1's sums first
    assert _defers(ch[3], pl[3]) and ch[3].ka_valid
    assert all(c.nt_big == 1 and not c.refused for n in G.CHAINS for c in [G.BY_NAME[x] for x in G.CHAINS[n]])


def test_size_limits_of_the_gpu_cases():
    for c in G.RUN_CASES:
        assert c.M == 32768 or (c.M <= 8192 and c.Ka <= 768 and c.Nb <= 768), c.name
    assert sum(c.M == 32768 for c in G.RUN_CASES) == 4          # one shape: the big-tile kernel with / without a row scale, and switched off


@pytest.mark.parametrize("name", [c.name for c in G.RUN_CASES])
def test_exact_inputs_keep_every_intermediate_exact_in_fp32(name):
    """every product and partial sum is a multiple of 1/4 and, by the sums of absolute values (pre-fill included), below 2^22: as a multiple of
    1/4 it needs fewer than 24 mantissa bits, whatever the order of summation"""
    c = G.BY_NAME[name]
    op = G.inputs(name, False)
    for n in ("A", "B", "W", "out0", "db0"):
        if n in op:
            assert np.array_equal(op[n], np.round(op[n])) and (n in ("out0", "db0") or np.abs(op[n]).max() <= 2), n
            assert n in ("out0", "db0", "W") or np.array_equal(G._store(op[n], c.dtA if n == "A" else c.dtB), op[n])
    for n in ("P", "Q"):
        if n in op:
            assert np.isin(op[n], G.PQ_SET).all()
    if "rs" in op:
        assert np.isin(op["rs"], G.RS_SET).all() and op["rs"][0] != op["rs"][1] and (len(op["rs"]) < 3 or (op["rs"] == 0).any())
    mag = G.magnitudes(c, op)
    ref = G.reference(c, op)
    assert set(mag) == set(ref)
    for n in mag:
        assert mag[n].max() * 4 < 2 ** 24, (n, mag[n].max())
        assert np.array_equal(ref[n] * 4, np.round(ref[n] * 4)), n
        assert np.array_equal(ref[n].astype(np.float32).astype(np.float64), ref[n]), n
