"""Shared by tests/test_ensemble.py, tests/test_ensemble_mutants.py and tests/test_ensemble_gpu.py: the case table of ishara_logits_combine,
a float32 numpy twin of the kernel's operation order with switchable mistakes, and the comparison with ishara_amd.ensemble.combine_reference.

The bound.  |got - ref| <= K * 2^-24 * scale[row], scale[row] = 1 + (max over the models read and the classes of |z|) + (max over the classes
of |ref|) of the row: every intermediate of the kernel (z, z - max z, the log-probabilities, their weighted sum) is at most a small multiple
of these magnitudes, and each fp32 operation rounds by at most 2^-24 relative.  K is not fitted to the device: K_HOST is the worst
err / (2^-24 * scale) of the unmutated fp32 twin against the fp64 reference over the whole case table, measured on the CPU (`measure_k_host`,
printed by tests/test_ensemble_mutants.py), and K = 4 * K_HOST; the factor covers the device's expf / logf, which may differ from numpy's by
an ulp or two each, fused multiply-adds, and a different but fixed reduction tree.  Rows past a clip's end must be +0 exactly.

A case is a dict: C, M, B, T, mode (0 / 1), kind ("normal": N(0, 1) logits, no temperatures; "big_t05" / "big_t2": some entries at +-80 and a
temperature of 0.5 / 2 for every model), weights (float32 [M], as the device gets them), logits (M float32 arrays [B, T, C]), inv_temp
(float32 [M] or None), temperatures, frame_len (int32 [B] or None).  A model whose weight is 0 holds NaN everywhere, and so do the rows past
the end of a clip under a mixed frame_len: neither may be read."""
import functools

import numpy as np

from ishara_amd.ensemble import combine_reference, inverse_temperatures

CLASSES = (2, 59, 60, 63, 64)
MODELS = (1, 2, 3, 8)
SHAPES = ((1, 1), (3, 5), (2, 67), (4, 176))          # row counts that are no multiple of any rows-per-workgroup choice
KINDS = ("normal", "big_t05", "big_t2")
WEIGHTS = ("uniform", "one_hot", "unequal", "zero")
FRAME_LEN = ("none", "full", "mix")
EPS = 2.0 ** -24
K_HOST = 2.4          # measured: see measure_k_host and DESIGN.md §3 (the worst case of the table, C 64 / M 8 / mode 0 / temperature 2, gives 2.375)
K = 4 * K_HOST
MUTANTS = ("weight_next", "no_temperature", "no_final_norm", "mode1_as_mode0", "no_max_subtraction", "pad_lanes_exp0", "zero_weight_read",
           "frame_len_off_by_one", "tail_unwritten")


def _weights(kind, M):
    if kind == "uniform":
        return np.full(M, 1.0 / M).astype(np.float32)
    if kind == "one_hot":
        w = np.zeros(M, np.float32)
        w[M // 2] = 1.0
        return w
    w = np.arange(1, M + 1, dtype=np.float64)
    if kind == "zero":
        w[(M - 1) // 2] = 0.0                             # M = 1: no weight > 0, the uniform row
    return (w / max(w.sum(), 1.0)).astype(np.float32)


def _frame_len(kind, B, T, i):
    if kind == "none":
        return None
    if kind == "full":
        return np.full(B, T, np.int32)
    vals = [0, 1, T - 1, T, T + 5, -3]
    return np.array([vals[(b + i) % len(vals)] for b in range(B)], np.int32)


def clip_frames(frame_len, B, T):
    """Tb per clip: T without frame_len, 0 for a value outside [1, T]"""
    if frame_len is None:
        return np.full(B, T, np.int64)
    fl = np.asarray(frame_len, np.int64)
    return np.where((fl < 1) | (fl > T), 0, fl)


def make_case(i, Cn, M, B, T, mode, kind, wkind, fkind):
    g = np.random.default_rng(9000 + i)
    xs = [g.standard_normal((B, T, Cn)).astype(np.float32) for _ in range(M)]
    temps = None
    if kind != "normal":
        for x in xs:
            hit = g.random(x.shape) < 0.08
            x[hit] = np.where(g.random(int(hit.sum())) < 0.5, 80.0, -80.0).astype(np.float32)
        temps = np.full(M, 0.5 if kind == "big_t05" else 2.0)
    w = _weights(wkind, M)
    fl = _frame_len(fkind, B, T, i)
    for m in range(M):
        if not w[m] > 0:
            xs[m][:] = np.nan
    if fkind == "mix":
        tb = clip_frames(fl, B, T)
        for x in xs:
            for b in range(B):
                x[b, tb[b]:] = np.nan
    for x in xs:
        x.setflags(write=False)
    return dict(name=f"{i:02d}-C{Cn}-M{M}-B{B}xT{T}-mode{mode}-{kind}-{wkind}-{fkind}", C=Cn, M=M, B=B, T=T, mode=mode, kind=kind, wkind=wkind, fkind=fkind,
                logits=xs, weights=w, temperatures=temps, inv_temp=inverse_temperatures(temps, M), frame_len=fl)


@functools.lru_cache(maxsize=None)
def cases():
    """Every class count x shape x mode, the other factors rotating through their values with strides that make every value meet both
    modes (checked below); then the all-zero weight vector and M = 8 in mode 1 with a zero weight at the largest shape."""
    out, i = [], 0
    for mode in (0, 1):
        for ci, Cn in enumerate(CLASSES):
            for si, (B, T) in enumerate(SHAPES):
                out.append(make_case(i, Cn, MODELS[(i + mode) % 4], B, T, mode, KINDS[(i + ci) % 3], WEIGHTS[(i // 2 + si + ci) % 4], FRAME_LEN[(i + i // 4) % 3]))
                i += 1
    for mode in (0, 1):
        c = make_case(i, 60, 3, 3, 5, mode, "normal", "uniform", "mix")
        c["weights"] = np.zeros(3, np.float32)
        c["name"] += "-allzero"
        out.append(c)
        i += 1
        out.append(make_case(i, 60, 8, 4, 176, mode, "big_t05", "zero", "mix"))
        i += 1
    for mode in (0, 1):
        sub = [c for c in out if c["mode"] == mode]
        for key, vals in (("C", CLASSES), ("M", MODELS), ("kind", KINDS), ("wkind", WEIGHTS), ("fkind", FRAME_LEN)):
            assert {c[key] for c in sub} == set(vals), (mode, key)
        assert {(c["B"], c["T"]) for c in sub} == set(SHAPES)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(ref float64 [B, T, C], scale float64 [B, T]) of a case, computed once and read-only"""
    c = next(c for c in cases() if c["name"] == name)
    ref = combine_reference(c["logits"], c["weights"], "linear" if c["mode"] else "log_linear", c["temperatures"], c["frame_len"])
    zmax = np.zeros((c["B"], c["T"]))
    with np.errstate(invalid="ignore"):
        for m in range(c["M"]):
            if c["weights"][m] > 0:
                z = np.abs(c["logits"][m].astype(np.float64) * (float(c["inv_temp"][m]) if c["inv_temp"] is not None else 1.0))
                zmax = np.fmax(zmax, np.nan_to_num(z, nan=0.0).max(axis=-1))        # NaN only past a clip's end, where no bound is needed
    scale = 1.0 + zmax + np.abs(ref).max(axis=-1)
    ref.setflags(write=False)
    scale.setflags(write=False)
    return ref, scale


def compare(case, got, k=K):
    """err / bound of `got` [B, T, C] against the fp64 reference: the largest |got - ref| / (k * 2^-24 * scale[row]) over the rows inside
    their clips; inf for a NaN there, and inf when a row past a clip's end is anything but +0.  <= 1 passes."""
    ref, scale = reference(case["name"])
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float32, (got.shape, got.dtype)
    inside = np.arange(case["T"])[None, :] < clip_frames(case["frame_len"], case["B"], case["T"])[:, None]
    tail = got[~inside]
    if tail.size and not ((tail == 0).all() and not np.signbit(tail).any()):
        return float("inf")
    if not inside.any():
        return 0.0
    err = np.abs(got.astype(np.float64) - ref).max(axis=-1)[inside]
    if not np.isfinite(err).all():
        return float("inf")
    return float((err / (k * EPS * scale[inside])).max())


# ---------------------------------------------------------------------------------------------------- the fp32 twin
_LANES = np.arange(64)


def _butterfly(v, op):
    for o in (32, 16, 8, 4, 2, 1):          # the xor butterfly of the kernel's wave_sum / wave_max: every lane ends with the same bits
        v = op(v, v[:, _LANES ^ o])
    return v


def twin(case, mutant=None):
    """ishara_logits_combine in float32 numpy, one row per wavefront and one class per lane as the kernel has them, same operation order
    (products and sums are rounded separately where the device may fuse them).  `mutant`: one of MUTANTS, a mistake the bound must reject."""
    assert mutant is None or mutant in MUTANTS, mutant
    f32 = np.float32
    Cn, M, B, T, mode = case["C"], case["M"], case["B"], case["T"], case["mode"]
    rows = B * T
    on = (_LANES < Cn)[None, :]
    w = case["weights"].astype(f32)
    if mutant == "weight_next":
        w = np.roll(w, 1)
    use = [bool(w[m] > 0) for m in range(M)]
    if mutant == "zero_weight_read":
        use = [True] * M
    it = None if (case["inv_temp"] is None or mutant == "no_temperature") else case["inv_temp"].astype(f32)
    if mutant == "mode1_as_mode0":
        mode = 0

    def log_softmax(z):
        mx = _butterfly(np.where(on, z, f32(-np.inf)), np.maximum) if mutant != "no_max_subtraction" else np.zeros_like(z)
        d = z - mx
        e = np.where(on, np.exp(d), f32(1.0 if mutant == "pad_lanes_exp0" else 0.0))
        return d - np.log(_butterfly(e, np.add))

    with np.errstate(all="ignore"):
        zs = []
        for m in range(M):
            z = np.zeros((rows, 64), f32)
            if use[m]:
                z[:, :Cn] = case["logits"][m].reshape(rows, Cn)
                if it is not None:
                    z = z * it[m]
            zs.append(z)
        s = np.zeros((rows, 64), f32)
        if mode == 0:
            for m in range(M):
                if use[m]:
                    s = s + w[m] * log_softmax(zs[m])
        elif any(use):
            terms = [(np.log(w[m]) if w[m] > 0 else f32(0)) + log_softmax(zs[m]) for m in range(M) if use[m]]
            a = terms[0]
            for t in terms[1:]:
                a = np.maximum(a, t)
            acc = np.zeros((rows, 64), f32)
            for t in terms:
                acc = acc + np.exp(t - a)
            s = a + np.log(acc)
        out = (s if mutant == "no_final_norm" else log_softmax(s))[:, :Cn].reshape(B, T, Cn).astype(f32)
    if case["frame_len"] is not None:
        tb = clip_frames(case["frame_len"], B, T) + (1 if mutant == "frame_len_off_by_one" else 0)
        past = np.arange(T)[None, :] >= tb[:, None]
        out[past] = np.nan if mutant == "tail_unwritten" else 0.0          # the tests poison `out` with NaN before the call
    return out


def measure_k_host():
    """the worst err / (2^-24 * scale) of the unmutated twin over the table: K_HOST must not be below it"""
    return max(compare(c, twin(c), k=1.0) for c in cases())
