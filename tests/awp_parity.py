"""Shared by tests/test_awp_gpu.py, tests/test_awp_mutants.py and tests/test_awp.py: the segment tables, the vectors with their variants
and the comparison of one ishara_awp_perturb (or a restatement of it) with train_state.awp_reference.

A result is a dict: w_adv, backup, g_after (float32 [n]), scale (float32 [S]) and stats {grad_norm, delta_norm, perturbed, zeroed}.
`compare` returns the list of what is wrong with it (empty: nothing):
  scale      within 1 fp32 ulp of the reference's (equality is expected; the ulp covers the order of the fp64 summation, which is the
             kernel's own: the reference's math.fsum is exactly rounded, a sum of n <= 2^20 fp64 terms in any order is within n * 2^-53
             relative of it, far below half an fp32 ulp except next to a rounding boundary)
  w_adv      bit for bit fp32(w + fp32(scale * g)) with the result's OWN scale on the segments the reference perturbs; on the segments the
             reference zeroes, the bits of w
  backup     the bits of w; g_after the bits of g
  perturbed, zeroed   exactly the reference's; a zeroed segment has scale 0
  grad_norm, delta_norm   within 1e-6 relative of the reference's

The vectors are N(0, 1) gradients and N(0, 0.25) weights: scale * g and the sum are far from the subnormal range, so the bit comparison
does not depend on a denormal mode."""
import functools

import numpy as np

from ishara_amd import train_state as TS

CHUNK = TS.AWP_CHUNK
DELTA, EPS = 0.2, 1e-4
TABLE_A = [1, 3, 4, 5, 1023, 1024, 1025, 4099, 2 * CHUNK + 7, 2, 64]      # offsets mostly unaligned; one segment of more than 2 chunks
TABLE_B = [5]
# more segments, hence more chunks, than the most workgroups of a launch: the second grid-stride round of every kernel, and more than
# one segment per thread in the two single-workgroup kernels
TABLE_D = [(1, 2, 3, 5, 7)[i % 5] for i in range(TS.GRAD_GRID_CAP + 52)] + [CHUNK + 1]
VARIANTS = ("plain", "zero_grad", "nonfinite", "huge")


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def table_c():
    """awp_segments of the entries of CFGS["tiny"] (tests/test_model_gpu.py), from a model without a device"""
    from ishara_amd import make_config
    from ishara_amd.model import Model
    from test_model_gpu import CFGS
    kw = {k: v for k, v in CFGS["tiny"].items() if k != "B"}
    m = Model(make_config(dropout_rate=0.0, head_dropout=0.0, conformer_attn_dropout=0.0, dtype="f32", max_batch=CFGS["tiny"]["B"], **kw), device=None)
    seg = TS.awp_segments(m.entries, m.n_train)
    seg.setflags(write=False)
    return seg


def table(name):
    return {"A": offsets(TABLE_A), "B": offsets(TABLE_B), "C": table_c(), "D": offsets(TABLE_D)}[name]


def variant_segments(seg_off):
    """the segments a variant touches: (zero_grad, nan, inf, huge), spread over the table (all the same one in a table of one segment)"""
    S = len(seg_off) - 1
    return (min(4, S - 1), min(6, S - 1), min(8, S - 1), min(7, S - 1))


@functools.lru_cache(maxsize=None)
def _base(n):
    r = np.random.default_rng(4000 + n % 9973)
    return (0.5 * r.standard_normal(n)).astype(np.float32), r.standard_normal(n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def vectors(name, variant="plain"):
    """(w, g) for a table and a variant, generated once (read-only)"""
    seg = table(name)
    w, g = (a.copy() for a in _base(int(seg[-1])))
    zs, ns, fs, hs = variant_segments(seg)
    if variant == "zero_grad":
        g[seg[zs]:seg[zs + 1]] = 0.0
    elif variant == "nonfinite":
        g[seg[fs + 1] - 1] = np.inf                  # the last element of one segment
        g[(seg[ns] + seg[ns + 1]) // 2] = np.nan     # the middle of another (the same one in a table of one segment)
    elif variant == "huge":
        g[seg[hs]:seg[hs + 1]] = np.float32(3e19)    # squares past fp32, the sum far inside fp64
    elif variant != "plain":
        raise KeyError(variant)
    for a in (w, g):
        a.setflags(write=False)
    return w, g


@functools.lru_cache(maxsize=None)
def reference(name, variant="plain", relative=False):
    w, g = vectors(name, variant)
    w_adv, scale, stats = TS.awp_reference(w, g, table(name), DELTA, EPS, relative)
    return dict(w_adv=w_adv, scale=scale, stats=stats, backup=w, g_after=g)


def ulps(a, b):
    """distance in fp32 representable values between two arrays of non-negative finite floats (a huge number where one is not)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return np.where(np.isfinite(a) & np.isfinite(b) & (a >= 0) & (b >= 0), d, 2 ** 40)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def recompute(w, g, seg_off, scale, zeroed_mask):
    """fp32(w + fp32(scale[s] * g)) per segment, the bits of w where the segment is zeroed"""
    out = np.array(w, dtype=np.float32)
    for s, (lo, hi) in enumerate(zip(seg_off[:-1], seg_off[1:])):
        if not zeroed_mask[s]:
            with np.errstate(over="ignore", invalid="ignore", under="ignore"):
                out[lo:hi] = w[lo:hi] + np.float32(scale[s]) * g[lo:hi]
    return out


def compare(got, name, variant="plain", relative=False):
    """what is wrong with `got` as a result of the case (see the module docstring) -> list of messages"""
    ref = reference(name, variant, relative)
    w, g = vectors(name, variant)
    seg = table(name)
    bad = []
    scale = np.asarray(got["scale"], np.float32)
    zero_ref = np.array([not _finite_segment(w, g, seg, s, relative) for s in range(len(seg) - 1)])
    if scale.shape != ref["scale"].shape:
        return [f"scale has shape {scale.shape}, the reference {ref['scale'].shape}"]
    d = ulps(scale, ref["scale"])
    if d.max() > 1:
        s = int(np.argmax(d))
        bad.append(f"scale[{s}] = {scale[s]!r}, the reference has {ref['scale'][s]!r} ({int((d > 1).sum())} segments beyond 1 ulp)")
    if np.any(scale[zero_ref] != 0):
        bad.append("a zeroed segment has a scale other than 0")
    want = recompute(w, g, seg, scale, zero_ref)
    for key, exp in (("w_adv", want), ("backup", w), ("g_after", g)):
        a, b = bits(got[key]), bits(exp)
        if a.shape != b.shape or not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0]) if a.shape == b.shape else -1
            bad.append(f"{key}[{i}] = {a[i]:#010x}, expected {b[i]:#010x} ({int((a != b).sum())} elements differ)" if i >= 0 else f"{key}: wrong size")
    st, rs = got["stats"], ref["stats"]
    for k in ("perturbed", "zeroed"):
        if int(st[k]) != rs[k]:
            bad.append(f"{k} = {st[k]}, the reference has {rs[k]}")
    for k in ("grad_norm", "delta_norm"):
        if not abs(float(st[k]) - rs[k]) <= 1e-6 * abs(rs[k]):
            bad.append(f"{k} = {st[k]!r}, the reference has {rs[k]!r}")
    return bad


def _finite_segment(w, g, seg, s, relative):
    lo, hi = int(seg[s]), int(seg[s + 1])
    return bool(np.isfinite(g[lo:hi]).all()) and (not relative or bool(np.isfinite(w[lo:hi]).all()))


def subnormal_intermediates(name, variant="plain", relative=False):
    """how many of scale * g and w + scale * g are subnormal in the reference's run of the case"""
    ref = reference(name, variant, relative)
    w, g = vectors(name, variant)
    seg = table(name)
    tiny, count = np.finfo(np.float32).tiny, 0
    for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        if not _finite_segment(w, g, seg, s, relative):
            continue
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            step = ref["scale"][s] * g[lo:hi]
            for x in (step, w[lo:hi] + step):
                count += int(((x != 0) & (np.abs(x) < tiny)).sum())
    return count
