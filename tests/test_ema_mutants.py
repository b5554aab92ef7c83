"""On the vectors and scenarios of tests/test_ema_gpu.py (ema_parity.py): the bit-equality check the GPU tests apply to
ishara_weight_average / ishara_weight_swap rejects each ordinary mistake of the update, the warm-up, the skipped step, the overwrite and the
swap, played on the host: a kernel that made one could not pass.  First the facts the vectors were chosen for: no intermediate of the
reference is subnormal on them, and every mutant changes at least one bit."""
import numpy as np
import pytest

import ema_parity as EP
from ishara_amd import train_state as TS

N_MUT = 1025           # one workgroup span and one more element: vector body and tail


def _skipped(kw):
    return kw["skip_nonfinite"] and kw["nonfinite"] > 0


def _finish(avg, theta, st, alpha, every, residue=0):
    st["updates"] += 1
    st["alpha"] = alpha
    st["overwrote"] = 1 if every > 0 and st["updates"] % every == residue else 0
    return (avg, avg.copy()) if st["overwrote"] else (avg, theta)


def two_products(avg, theta, st, momentum, **kw):
    """m * avg + (1 - m) * theta"""
    if _skipped(kw):
        return TS.ema_reference(avg, theta, st, momentum, **kw)
    alpha = TS.ema_alpha(st["updates"], momentum, kw["warmup"])
    m = np.float32(1.0 - np.float64(alpha))
    return _finish(m * avg + alpha * theta, theta, st, alpha, kw["overwrite_every"])


def fused(avg, theta, st, momentum, **kw):
    """fma(alpha, theta - avg, avg): the product is exact in fp64 (24 + 24 bits), one rounding of the sum"""
    if _skipped(kw):
        return TS.ema_reference(avg, theta, st, momentum, **kw)
    alpha = TS.ema_alpha(st["updates"], momentum, kw["warmup"])
    diff = theta - avg
    new = (np.float64(alpha) * diff.astype(np.float64) + avg.astype(np.float64)).astype(np.float32)
    return _finish(new, theta, st, alpha, kw["overwrite_every"])


def warmup_one_ahead(avg, theta, st, momentum, **kw):
    """n + 1 in the warm-up rule"""
    if _skipped(kw):
        return TS.ema_reference(avg, theta, st, momentum, **kw)
    alpha = TS.ema_alpha(st["updates"] + 1, momentum, kw["warmup"])
    return _finish(avg + alpha * (theta - avg), theta, st, alpha, kw["overwrite_every"])


def update_on_skip(avg, theta, st, momentum, **kw):
    """the average moves on a skipped step (the counter and the record behave)"""
    if not _skipped(kw):
        return TS.ema_reference(avg, theta, st, momentum, **kw)
    alpha = TS.ema_alpha(st["updates"], momentum, kw["warmup"])
    st["overwrote"] = 0
    return avg + alpha * (theta - avg), theta


def counter_on_skip(avg, theta, st, momentum, **kw):
    """a skipped step writes nothing but advances the counter"""
    out = TS.ema_reference(avg, theta, st, momentum, **kw)
    if _skipped(kw):
        st["updates"] += 1
    return out


def overwrite_one_late(avg, theta, st, momentum, **kw):
    """the overwrite fires at updates % N == 1"""
    if _skipped(kw):
        return TS.ema_reference(avg, theta, st, momentum, **kw)
    alpha = TS.ema_alpha(st["updates"], momentum, kw["warmup"])
    return _finish(avg + alpha * (theta - avg), theta, st, alpha, kw["overwrite_every"], residue=1 if kw["overwrite_every"] > 1 else 0)


MUTANTS = {"two_products": two_products, "fused": fused, "warmup_one_ahead": warmup_one_ahead, "update_on_skip": update_on_skip,
           "counter_on_skip": counter_on_skip, "overwrite_one_late": overwrite_one_late}


def test_no_intermediate_is_subnormal():
    for n in (s for s in EP.SIZES if s <= EP.SPAN + 1):
        for name, sc in EP.SCENARIOS.items():
            assert EP.subnormal_intermediates(n, sc) == 0, (n, name)
    assert EP.subnormal_intermediates(EP.SIZES[-1], EP.SCENARIOS["ordering"]) == 0        # the largest size, its longest scenario


def test_the_reference_passes_its_own_check():
    for name, sc in EP.SCENARIOS.items():
        assert EP.same(EP.play(TS.ema_reference, N_MUT, sc), EP.reference(N_MUT, name)), name


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_bit_equality_rejects_the_mistake(mut):
    rejected = {}
    for name, sc in EP.SCENARIOS.items():
        got, want = EP.play(MUTANTS[mut], N_MUT, sc), EP.reference(N_MUT, name)
        if not EP.same(got, want):
            rejected[name] = EP.first_difference(got, want)
    print(mut, rejected)
    assert rejected, f"{mut}: no scenario of the GPU test tells it from the reference"
    need = {"two_products": "plain", "fused": "plain", "warmup_one_ahead": "warmup", "update_on_skip": "skipped", "counter_on_skip": "skipped",
            "overwrite_one_late": "overwrite2"}[mut]
    assert need in rejected, f"{mut}: the scenario written for it ({need}) does not reject it"
    bits = [name for name in rejected if any(g["avg"] != w["avg"] or g["theta"] != w["theta"] or g["alpha"] != w["alpha"] or g["updates"] != w["updates"]
                                             for g, w in zip(EP.play(MUTANTS[mut], N_MUT, EP.SCENARIOS[name]), EP.reference(N_MUT, name)))]
    assert bits, f"{mut}: changes no bit of avg, theta, alpha or the counter"


def test_rounding_mutants_change_many_elements():
    """the two rounding mistakes are not told apart by a lucky element: each flips the last bit of a good share of 1025 elements"""
    want = np.frombuffer(EP.reference(N_MUT, "plain")[0]["avg"], np.uint32)
    for mut in ("two_products", "fused"):
        got = np.frombuffer(EP.play(MUTANTS[mut], N_MUT, EP.SCENARIOS["plain"])[0]["avg"], np.uint32)
        changed = int((got != want).sum())
        print(mut, changed, "of", N_MUT, "elements differ after one launch")
        assert changed >= N_MUT // 50


def test_swap_check_rejects_a_copy():
    for n in EP.SIZES[:-1]:
        a0, b0 = EP.bit_patterns(n)
        assert (a0 != b0).all(), n
        assert EP.swap_same(b0.copy(), a0.copy(), a0, b0)                        # the exchange
        assert not EP.swap_same(b0.copy(), b0.copy(), a0, b0)                    # a = b, b left alone
        assert not EP.swap_same(a0.copy(), a0.copy(), a0, b0)                    # b = a
        assert not EP.swap_same(a0.copy(), b0.copy(), a0, b0)                    # nothing happened
    a0, b0 = EP.bit_patterns(1025)
    f = a0.view(np.float32)
    assert np.isnan(f).sum() >= 4 and np.isinf(f).sum() >= 2                     # quiet and signalling NaNs with payloads, both infinities
