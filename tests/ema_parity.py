"""Shared by tests/test_ema_gpu.py and tests/test_ema_mutants.py: the vectors, the launch scenarios and the bit-equality check of
ishara_weight_average / ishara_weight_swap against train_state.ema_reference.

A scenario is a list of launches on one pair of buffers; launch k is handed thetas[k % 3] (freshly written into the theta buffer, except
in the `ordering` scenario, whose launches run back to back on what the buffers hold).  A play of a scenario is the list of snapshots
taken after every launch: the bytes of avg and theta and the three fields of the record.  `same` compares two plays in every bit.

The vectors are N(0, 1): theta - avg, alpha * (theta - avg) and the sum are far from the subnormal range (`subnormal_intermediates`
counts them; the mutants file asserts the count is 0), so the comparison does not depend on a denormal mode."""
import functools

import numpy as np

from ishara_amd import train_state as TS

SPAN, CAP = TS.GRAD_WG_SPAN, TS.GRAD_GRID_CAP
SIZES = sorted({1, 3, 4, 5, 255, 257, 1023, 1025, SPAN + 1, CAP * SPAN + 5})      # the last one: a second grid-stride round
MOMENTUM = 0.9

# launches: (nonfinite of the grad-stats record, skip_nonfinite)
SCENARIOS = {
    "plain": dict(warmup=False, every=0, launches=[(0, 0)] * 3),
    "warmup": dict(warmup=True, every=0, launches=[(0, 0)] * 3),
    "overwrite2": dict(warmup=True, every=2, launches=[(0, 0)] * 4),
    "skipped": dict(warmup=True, every=0, launches=[(0, 0), (1, 1), (1, 0)]),        # a step, a skipped one, the record without the guard
    "skipped_overwrite": dict(warmup=False, every=2, launches=[(0, 0), (1, 1), (0, 0), (0, 0)]),
    "ordering": dict(warmup=True, every=0, launches=[(0, 0)] * 50, same_theta=True),
}


@functools.lru_cache(maxsize=None)
def vectors(n):
    """(avg0, [theta_0, theta_1, theta_2]) for a size, generated once (read-only)"""
    g = np.random.default_rng(1000 + n % 9973)
    out = [g.standard_normal(n).astype(np.float32) for _ in range(4)]
    for a in out:
        a.setflags(write=False)
    return out[0], out[1:]


def snap(avg, theta, state):
    return dict(avg=np.asarray(avg, np.float32).tobytes(), theta=np.asarray(theta, np.float32).tobytes(), updates=int(state["updates"]),
                alpha=np.float32(state["alpha"]).tobytes(), overwrote=int(state["overwrote"]))


def play(impl, n, sc):
    """the scenario on the host through `impl` (the signature of train_state.ema_reference) -> snapshots"""
    avg0, thetas = vectors(n)
    avg, theta, st, out = avg0.copy(), None, TS.ema_state_init(), []
    for k, (nonfinite, skip) in enumerate(sc["launches"]):
        if theta is None or not sc.get("same_theta"):
            theta = thetas[k % 3].copy()
        avg, theta = impl(avg, theta, st, MOMENTUM, warmup=sc["warmup"], overwrite_every=sc["every"], nonfinite=nonfinite, skip_nonfinite=bool(skip))
        out.append(snap(avg, theta, st))
    return out


@functools.lru_cache(maxsize=None)
def reference(n, name):
    return play(TS.ema_reference, n, SCENARIOS[name])


def same(got, want):
    """two plays agree in every bit of every snapshot"""
    return len(got) == len(want) and all(g == w for g, w in zip(got, want))


def first_difference(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        for f in ("updates", "alpha", "overwrote", "avg", "theta"):
            if g[f] != w[f]:
                if f in ("avg", "theta"):
                    a, b = np.frombuffer(g[f], np.uint32), np.frombuffer(w[f], np.uint32)
                    i = int(np.flatnonzero(a != b)[0])
                    return f"launch {k + 1}: {f}[{i}] = {a[i]:#010x}, the reference has {b[i]:#010x} ({int((a != b).sum())} elements differ)"
                return f"launch {k + 1}: {f} = {g[f]!r}, the reference has {w[f]!r}"
    return "no difference" if len(got) == len(want) else f"{len(got)} snapshots, the reference has {len(want)}"


def subnormal_intermediates(n, sc):
    """how many of theta - avg, alpha * (theta - avg) and the sum are subnormal anywhere in the reference's play of the scenario"""
    tiny = np.finfo(np.float32).tiny
    count = [0]

    def spy(avg, theta, st, momentum, **kw):
        if not (kw["skip_nonfinite"] and kw["nonfinite"] > 0):
            alpha = TS.ema_alpha(st["updates"], momentum, kw["warmup"])
            diff = theta - avg
            prod = alpha * diff
            for x in (diff, prod, avg + prod):
                count[0] += int(((x != 0) & (np.abs(x) < tiny)).sum())
        return TS.ema_reference(avg, theta, st, momentum, **kw)
    play(spy, n, sc)
    return count[0]


# ---------------------------------------------------------------------------------- the swap
@functools.lru_cache(maxsize=None)
def bit_patterns(n):
    """two [n] arrays of random 32-bit words (as uint32; NaNs with payloads, signalling NaNs and infinities among them)"""
    g = np.random.default_rng(77 + n % 9973)
    a = g.integers(0, 2 ** 32, size=n, dtype=np.uint32)
    b = g.integers(0, 2 ** 32, size=n, dtype=np.uint32)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff80abcd, 0x7f800000, 0xff800000, 0x00000001, 0x80000000], dtype=np.uint32)
    for j, w in enumerate(special[:n]):            # the specials in a's leading words; in b's last ones with another mantissa bit, so a != b
        a[j] = w
        b[n - 1 - j] = w ^ np.uint32(0x100)
    for x in (a, b):
        x.setflags(write=False)
    return a, b


def swap_same(got_a, got_b, a0, b0):
    """after one swap: a holds b's earlier words and b holds a's"""
    return got_a.tobytes() == b0.tobytes() and got_b.tobytes() == a0.tobytes()
