"""Shared by tests/test_param_groups_gpu.py, tests/test_param_groups_mutants.py and tests/test_param_groups.py: the segment tables (those
of awp_parity.py), the row assignments, the vectors with their variants and the comparison of one grouped optimizer step.

A case is (table, assignment, iteration, variant).  A result is a dict: theta, m, v, slow (float32 [n]) and rec, the 16-byte record as
(coef, nonfinite, skipped) or None when the case runs without one.  `compare(got, expected)` works on bits: the four arrays word for
word, the record exactly; it returns the list of what is wrong (empty: nothing).

Row assignments over ROWS = [(1, 1, 0), (0.25, 1, 0), (1, 0, 0), frozen, (0, 1, 0), (3, 0.5, 0)] (lr_scale, wd_scale, frozen):
  cycle    segment s takes row s % 6: neighbours always differ, so a segment lookup off by one shows
  shifted  row (s + 3) % 6: a segment frozen in one of the two is scaled in the other
  ends     row (s + 1) % 6, but the first, the last and the longest segment frozen (in table A neither cycle nor shifted freezes the last
           or the long segment: this one does, and the other two scale them)
  default  every row (1, 1, 0)
Iterations 1 (no rectification, no Lookahead sync), 5 (the first rectified step, and a sync) and 6 (rectified, no sync); there is no
step with a sync and without rectification (test_param_groups.py checks this with train_state.radam_coeffs).
Variants:
  plain             no record
  inf_theta         one +Inf weight in a segment whose row has wd_scale = 0: wd * 0 must be a step without decay, not + 0 * theta (NaN);
                    a record with coef 0.75, nonfinite 0 and the skip switch on (a switch that is not taken)
  nan_frozen_grad   a NaN in a frozen segment's gradient: nothing of it may reach any slot; the same record
  nonfinite_skip    a record with nonfinite = 2, skipped = 7 and the skip switch: nothing is written, skipped becomes 8
The CPU expectation is train_state.param_groups_reference; the GPU tests build theirs from the plain operator (see there)."""
import functools

import numpy as np

import awp_parity as AP
from ishara_amd import train_state as TS

CHUNK = TS.AWP_CHUNK
LR, WD = 4e-3, 0.01
ROWS = [(1.0, 1.0, 0), (0.25, 1.0, 0), (1.0, 0.0, 0), (1.0, 1.0, 1), (0.0, 1.0, 0), (3.0, 0.5, 0)]
TABLES = ("A", "B", "C", "D")
ASSIGNMENTS = ("cycle", "shifted", "ends", "default")
ITERATIONS = (1, 5, 6)
VARIANTS = ("plain", "inf_theta", "nan_frozen_grad", "nonfinite_skip")
COEF = 0.75

table = AP.table
bits = AP.bits


@functools.lru_cache(maxsize=None)
def rows(name, assignment):
    """the PARAM_GROUP_DTYPE rows of a table under an assignment (read-only)"""
    S = len(table(name)) - 1
    shift = {"cycle": 0, "shifted": 3, "ends": 1}.get(assignment)
    if shift is None and assignment != "default":
        raise KeyError(assignment)
    r = np.zeros(S, dtype=TS.PARAM_GROUP_DTYPE)
    for s in range(S):
        r[s] = ROWS[0] + (0,) if shift is None else ROWS[(s + shift) % 6] + (0,)
    if assignment == "ends":
        for s in (0, S - 1, int(np.argmax(np.diff(table(name))))):
            r[s] = ROWS[3] + (0,)
    r.setflags(write=False)
    return r


def segment_with(name, assignment, want):
    """the first segment whose row is `want` ("frozen" or "no_decay"), or None"""
    for s, r in enumerate(rows(name, assignment)):
        if want == "frozen" and r["frozen"] != 0:
            return s
        if want == "no_decay" and r["frozen"] == 0 and r["wd_scale"] == 0:
            return s
    return None


def applies(name, assignment, variant):
    """inf_theta needs an unfrozen segment without decay, nan_frozen_grad a frozen one"""
    if variant == "inf_theta":
        return segment_with(name, assignment, "no_decay") is not None
    if variant == "nan_frozen_grad":
        return segment_with(name, assignment, "frozen") is not None
    return variant in VARIANTS


CASES = [(t, a, v) for t in TABLES for a in ASSIGNMENTS for v in VARIANTS if applies(t, a, v)]


@functools.lru_cache(maxsize=None)
def _base(n):
    r = np.random.default_rng(7000 + n % 9973)
    theta = (0.5 * r.standard_normal(n)).astype(np.float32)
    grad = r.standard_normal(n).astype(np.float32)
    m = (0.1 * r.standard_normal(n)).astype(np.float32)
    v = (0.01 + 0.1 * r.random(n)).astype(np.float32)
    slow = (theta + 0.01 * r.standard_normal(n)).astype(np.float32)
    return theta, grad, m, v, slow


@functools.lru_cache(maxsize=None)
def vectors(name, assignment="cycle", variant="plain"):
    """dict(theta, grad, m, v, slow, rec, skip) of a case, generated once (read-only); rec = (coef, nonfinite, skipped) or None"""
    seg = table(name)
    theta, grad, m, v, slow = (a.copy() for a in _base(int(seg[-1])))
    rec, skip = None, False
    if variant == "inf_theta":
        s = segment_with(name, assignment, "no_decay")
        theta[(seg[s] + seg[s + 1]) // 2] = np.inf
        rec, skip = (COEF, 0, 7), True
    elif variant == "nan_frozen_grad":
        s = segment_with(name, assignment, "frozen")
        grad[seg[s]] = np.nan
        grad[seg[s + 1] - 1] = np.nan
        rec, skip = (COEF, 0, 7), True
    elif variant == "nonfinite_skip":
        rec, skip = (COEF, 2, 7), True
    elif variant != "plain":
        raise KeyError(variant)
    for a in (theta, grad, m, v, slow):
        a.setflags(write=False)
    return dict(theta=theta, grad=grad, m=m, v=v, slow=slow, rec=rec, skip=skip)


@functools.lru_cache(maxsize=None)
def expected(name, assignment, iteration, variant="plain"):
    """the result train_state.param_groups_reference gives the case"""
    c = vectors(name, assignment, variant)
    st = dict(m=c["m"].copy(), v=c["v"].copy(), slow=c["slow"].copy(), step=iteration - 1, skipped=c["rec"][2] if c["rec"] else 0)
    coef, nonfinite = (c["rec"][0], c["rec"][1]) if c["rec"] else (1.0, 0)
    theta = TS.param_groups_reference(c["theta"].copy(), c["grad"], st, table(name), rows(name, assignment), LR, coef=coef, nonfinite=nonfinite,
                                      skip_nonfinite=c["skip"], weight_decay=WD)
    return dict(theta=theta, m=st["m"], v=st["v"], slow=st["slow"], rec=(coef, nonfinite, st["skipped"]) if c["rec"] else None)


def compare(got, exp):
    """what is wrong with `got` against `exp`, on bits -> list of messages"""
    bad = []
    for key in ("theta", "m", "v", "slow"):
        a, b = bits(got[key]), bits(exp[key])
        if a.shape != b.shape:
            bad.append(f"{key}: wrong size {a.shape}, expected {b.shape}")
        elif not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0])
            bad.append(f"{key}[{i}] = {a[i]:#010x}, expected {b[i]:#010x} ({int((a != b).sum())} elements differ)")
    g, e = got.get("rec"), exp.get("rec")
    if (g is None) != (e is None):
        bad.append(f"rec = {g!r}, expected {e!r}")
    elif e is not None:
        if bits(np.float32(g[0])) != bits(np.float32(e[0])):
            bad.append(f"rec.coef = {g[0]!r}, expected {e[0]!r}")
        if int(g[1]) != int(e[1]):
            bad.append(f"rec.nonfinite = {g[1]}, expected {e[1]}")
        if int(g[2]) != int(e[2]):
            bad.append(f"rec.skipped = {g[2]}, expected {e[2]}")
    return bad


# ---------------------------------------------------------------------------------- the gradient mask
@functools.lru_cache(maxsize=None)
def mask_gradient(name, assignment):
    """a gradient with NaN, Inf and -0.0 at the first, a middle and the last element of a frozen and of an unfrozen segment (read-only)"""
    seg = table(name)
    r = rows(name, assignment)
    g = _base(int(seg[-1]))[1].copy()
    specials = np.array([np.nan, np.inf, -0.0], dtype=np.float32)
    for frozen in (True, False):
        hits = [s for s in range(len(r)) if (r[s]["frozen"] != 0) == frozen]
        for j, s in enumerate(hits[:3] + hits[-3:]):
            lo, hi = int(seg[s]), int(seg[s + 1])
            for k, i in enumerate((lo, (lo + hi) // 2, hi - 1)):
                g[i] = specials[(j + k) % 3]
    g.setflags(write=False)
    return g


def compare_mask(got, exp):
    a, b = bits(got), bits(exp)
    if a.shape != b.shape:
        return [f"g: wrong size {a.shape}, expected {b.shape}"]
    if not np.array_equal(a, b):
        i = int(np.flatnonzero(a != b)[0])
        return [f"g[{i}] = {a[i]:#010x}, expected {b[i]:#010x} ({int((a != b).sum())} words differ)"]
    return []
