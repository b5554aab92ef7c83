"""Shared by tests/test_kd.py, tests/test_kd_mutants.py and tests/test_kd_gpu.py: the case table of ishara_kd_grad, a float32 numpy twin of the
kernel's operation order with switchable mistakes, and the comparison with ishara_amd.kd.kd_reference (numpy fp64).

The bounds, after tests/ensemble_parity.py.  With scale[row] = 1 + inv_temp * (max_c |z| + max_c |u|) of the row,
    |G - G_ref|   <= |grad_scale| * w_b * K * 2^-24 * scale[row]
    |KL - KL_ref| <= K_KL * 2^-24 * scale[row]
Every intermediate of the kernel (a = z * inv_temp, a - max a, the log-probabilities) is at most a small multiple of scale, each fp32 operation
rounds by at most 2^-24 relative, the probabilities are at most 1 and the teacher's sum to 1, so both errors grow linearly with scale.  The
constants are not fitted to the device: K_HOST and K_HOST_KL are the worst err / (2^-24 * scale ...) of the unmutated fp32 twin against the
fp64 reference over the whole case table, measured on the CPU (`measure_k_host`, printed by tests/test_kd_mutants.py), and K = 4 * K_HOST,
K_KL = 4 * K_HOST_KL; the factor covers the device's expf / logf, which may differ from numpy's by an ulp or two each.  Rows past a clip's end
must be +0 exactly (accumulate 0) or the old bits (accumulate 1).  With accumulate 1 the one fp32 addition adds 2^-24 * |old + G_ref|.

A case is a dict: C, B, T, mode (0 / 1), inv_temp (a float32 value), grad_scale (a float32 value), kind ("normal": N(0, 1) rows; "big": some
entries of both rows at +-80; "same": the teacher is a copy of the logits; "logprob": the teacher's rows are normalised log-probabilities),
fkind / frame_len (int32 [B] or None), logits and teacher (float32 [B, T, C], read-only).  Under a mixed frame_len the rows past a clip's end
hold NaN in both inputs: they may not be read."""
import functools

import numpy as np

from ishara_amd.kd import clip_frames, kd_reference

CLASSES = (2, 5, 59, 60, 64)
FRAMES = (1, 4, 5, 15, 16, 17, 33, 64, 65)            # around the wave's stride (4), the workgroup's 16 frames and kl_clip's 64-frame loads
BATCHES = (1, 2, 3)
INV_TEMPS = (1.0, 0.5, 0.25, 2.0)
KINDS = ("normal", "big", "same", "logprob")
FRAME_LEN = ("none", "full", "mix")
GRAD_SCALES = (1.0, 0.37, 1.0 / 64)
EPS = 2.0 ** -24
K_HOST = 1.0          # measured 0.955: see measure_k_host and DESIGN.md §3
K_HOST_KL = 2.7       # measured 2.601
K = 4 * K_HOST
K_KL = 4 * K_HOST_KL
MUTANTS = ("temperature_one_side", "pt_minus_ps", "no_wb", "inv_T_for_inv_Tb", "kl_reversed", "tail_written_accumulate", "dlb_from_G",
           "frame_len_off_by_one")


def _frame_len(kind, B, T, i):
    if kind == "none":
        return None
    if kind == "full":
        return np.full(B, T, np.int32)
    vals = [0, 1, T - 1, T, T + 1, -3]
    return np.array([vals[(b + i) % len(vals)] for b in range(B)], np.int32)


def _log_softmax32(x):
    x = x.astype(np.float64)
    d = x - x.max(axis=-1, keepdims=True)
    return (d - np.log(np.exp(d).sum(axis=-1, keepdims=True))).astype(np.float32)


def make_case(i, Cn, B, T, mode, inv_temp, kind, fkind, grad_scale):
    g = np.random.default_rng(26000 + i)
    z = g.standard_normal((B, T, Cn)).astype(np.float32)
    u = g.standard_normal((B, T, Cn)).astype(np.float32)
    if kind == "big":
        for x in (z, u):
            hit = g.random(x.shape) < 0.15
            x[hit] = np.where(g.random(int(hit.sum())) < 0.5, 80.0, -80.0).astype(np.float32)
    elif kind == "same":
        u = z.copy()
    elif kind == "logprob":
        u = _log_softmax32(3.0 * u)
    fl = _frame_len(fkind, B, T, i)
    if fkind == "mix":
        tb = clip_frames(fl, B, T)
        for b in range(B):
            z[b, tb[b]:] = np.nan
            u[b, tb[b]:] = np.nan
    z.setflags(write=False)
    u.setflags(write=False)
    return dict(name=f"{i:03d}-C{Cn}-B{B}xT{T}-mode{mode}-it{inv_temp:g}-{kind}-{fkind}", C=Cn, B=B, T=T, mode=mode, inv_temp=float(np.float32(inv_temp)),
                kind=kind, fkind=fkind, frame_len=fl, grad_scale=float(np.float32(grad_scale)), logits=z, teacher=u)


@functools.lru_cache(maxsize=None)
def cases():
    """Every class count x frame count x mode, the other factors rotating through their values with strides that make every value meet
    both modes (checked below)."""
    out, i = [], 0
    for mode in (0, 1):
        for ci, Cn in enumerate(CLASSES):
            for ti, T in enumerate(FRAMES):
                out.append(make_case(i, Cn, BATCHES[(i + ci) % 3], T, mode, INV_TEMPS[(i + mode) % 4], KINDS[(i // 2 + ci) % 4], FRAME_LEN[(i + i // 4 + mode) % 3],
                                     GRAD_SCALES[(i + ti) % 3]))
                i += 1
    for mode in (0, 1):
        sub = [c for c in out if c["mode"] == mode]
        for key, vals in (("C", CLASSES), ("T", FRAMES), ("B", BATCHES), ("kind", KINDS), ("fkind", FRAME_LEN)):
            assert {c[key] for c in sub} == set(vals), (mode, key)
        assert {c["inv_temp"] for c in sub} == set(INV_TEMPS), mode
    return tuple(out)


def frames_of(case):
    return clip_frames(case["frame_len"], case["B"], case["T"])


def inside_of(case):
    return np.arange(case["T"])[None, :] < frames_of(case)[:, None]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(kd_reference's dict in float64, scale float64 [B, T]) of a case, computed once and read-only"""
    c = next(c for c in cases() if c["name"] == name)
    ref = kd_reference(c["logits"], c["teacher"], c["inv_temp"], c["mode"], c["frame_len"], c["grad_scale"])
    with np.errstate(invalid="ignore"):
        zmax = np.nan_to_num(np.abs(c["logits"].astype(np.float64)), nan=0.0).max(axis=-1)       # NaN only past a clip's end, where no bound is needed
        umax = np.nan_to_num(np.abs(c["teacher"].astype(np.float64)), nan=0.0).max(axis=-1)
    scale = 1.0 + c["inv_temp"] * (zmax + umax)
    for v in list(ref.values()) + [scale]:
        v.setflags(write=False)
    return ref, scale


def _ratio(err, bound, inside):
    if not inside.any():
        return 0.0
    err = err[inside]
    if not np.isfinite(err).all():
        return float("inf")
    return float((err / bound[inside]).max())


def _tail_is_plus_zero(got, inside):
    tail = got[~inside]
    return (not tail.size) or ((tail == 0).all() and not np.signbit(tail).any())


def compare_grad(case, got, k=K, old=None):
    """err / bound of dlogits [B, T, C] against the fp64 reference over the rows inside their clips: <= 1 passes.  old None: an accumulate 0
    run, rows past a clip's end must be +0; old given: an accumulate 1 run on it, those rows must hold old's bits.  inf for a NaN inside a
    clip or a wrong row past its end."""
    ref, scale = reference(case["name"])
    got = np.asarray(got)
    assert got.shape == ref["grad"].shape and got.dtype == np.float32, (got.shape, got.dtype)
    inside = inside_of(case)
    want = ref["grad"]
    bound = abs(case["grad_scale"]) * ref["w"][:, None] * k * EPS * scale
    if old is None:
        if not _tail_is_plus_zero(got, inside):
            return float("inf")
    else:
        old = np.asarray(old, np.float32)
        if not np.array_equal(got[~inside].view(np.uint32), old[~inside].view(np.uint32)):
            return float("inf")
        want = np.where(inside[..., None], old.astype(np.float64) + want, 0.0)
        bound = bound + EPS * np.abs(want).max(axis=-1)
    return _ratio(np.abs(got.astype(np.float64) - want).max(axis=-1), bound, inside)


def compare_kl(case, got, k=K_KL):
    """err / bound of kl_frame [B, T]; rows past a clip's end must be +0"""
    ref, scale = reference(case["name"])
    got = np.asarray(got)
    assert got.shape == ref["kl_frame"].shape and got.dtype == np.float32, (got.shape, got.dtype)
    inside = inside_of(case)
    if not _tail_is_plus_zero(got, inside):
        return float("inf")
    return _ratio(np.abs(got.astype(np.float64) - ref["kl_frame"]), k * EPS * scale, inside)


def clip_sum(kl_frame, case):
    """kl_clip as the contract states it, from kl_frame's float32 values: the ascending sum from +0, in mode 1 times 1 / (float)Tb"""
    f32 = np.float32
    kl_frame = np.asarray(kl_frame, f32)
    out = np.zeros(case["B"], f32)
    for b, tb in enumerate(frames_of(case)):
        acc = f32(0.0)
        for t in range(kl_frame.shape[1]):
            acc = f32(acc + kl_frame[b, t])
        if case["mode"] == 1 and tb > 0:
            acc = f32(acc * (f32(1.0) / f32(tb)))
        out[b] = acc
    return out


def bf16_rne(x):
    """the bf16 bits (uint16) of float32 values by round-to-nearest-even; finite inputs"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def dlb_of(rows):
    """the padded bf16 copy of final dlogits rows [B, T, C]: uint32 [B * T, 64], class 2j in the low half of word j, zero past C"""
    rows = np.asarray(rows, np.float32)
    B, T, Cn = rows.shape
    h = np.zeros((B * T, 128), np.uint16)
    h[:, :Cn] = bf16_rne(rows.reshape(B * T, Cn))
    return (h[:, 0::2].astype(np.uint32) | (h[:, 1::2].astype(np.uint32) << 16))


# ---------------------------------------------------------------------------------------------------- the fp32 twin
_LANES = np.arange(64)


def _butterfly(v, op):
    for o in (32, 16, 8, 4, 2, 1):          # the xor butterfly of the kernel's wave_sum / wave_max: every lane ends with the same bits
        v = op(v, v[:, _LANES ^ o])
    return v


def twin(case, mutant=None, old=None):
    """ishara_kd_grad in float32 numpy, one row per wavefront and one class per lane as the kernel has them, same operation order, every
    product and sum rounded separately.  old: None for accumulate 0, else the float32 [B, T, C] dlogits an accumulate 1 call starts from.
    Returns dict(dlogits [B, T, C], dlb uint32 [B * T, 64], kl_frame [B, T], kl_clip [B]).  `mutant`: one of MUTANTS, a mistake the checks
    must reject."""
    assert mutant is None or mutant in MUTANTS, mutant
    f32 = np.float32
    Cn, B, T, mode = case["C"], case["B"], case["T"], case["mode"]
    rows = B * T
    on = (_LANES < Cn)[None, :]
    it, gs = f32(case["inv_temp"]), f32(case["grad_scale"])
    tb = frames_of(case)
    if mutant == "frame_len_off_by_one":
        tb = np.where((tb > 0) & (tb < T), tb + 1, tb)
    inside = (np.arange(T)[None, :] < tb[:, None]).reshape(rows)

    def row(x, inv_temp):
        a = np.zeros((rows, 64), f32)
        a[:, :Cn] = x.reshape(rows, Cn)
        a = a * inv_temp
        mx = _butterfly(np.where(on, a, f32(-np.inf)), np.maximum)
        d = a - mx
        e = np.where(on, np.exp(d), f32(0.0))
        s = _butterfly(e, np.add)
        return d - np.log(s), e / s

    with np.errstate(all="ignore"):
        lps, ps = row(case["logits"], it)
        lpt, pt = row(case["teacher"], f32(1.0) if mutant == "temperature_one_side" else it)
        term = ps * (lps - lpt) if mutant == "kl_reversed" else pt * (lpt - lps)
        kl = _butterfly(np.where(on, term, f32(0.0)), np.add)[:, 0]
        d = (pt - ps) if mutant == "pt_minus_ps" else (ps - pt)
        if mode == 1 and mutant != "no_wb":
            den = np.full(B, T) if mutant == "inv_T_for_inv_Tb" else np.maximum(tb, 1)
            wb = (f32(1.0) / den.astype(f32)).astype(f32)
            d = np.repeat(wb, T)[:, None] * d
        G = (gs * d)[:, :Cn]
    kl_frame = np.where(inside, kl, f32(0.0)).astype(f32).reshape(B, T)
    if old is None:
        final = np.where(inside[:, None], G, f32(0.0)).astype(f32)
    else:
        o = np.asarray(old, f32).reshape(rows, Cn)
        with np.errstate(all="ignore"):
            final = np.where(inside[:, None], o + G, (o + f32(1.0)) if mutant == "tail_written_accumulate" else o).astype(f32)
    final = final.reshape(B, T, Cn)
    dlb = dlb_of(np.where(inside.reshape(B, T)[..., None], G.reshape(B, T, Cn), f32(0.0)).astype(f32) if mutant == "dlb_from_G" else final)
    kc = dict(case, frame_len=None if case["frame_len"] is None else tb.astype(np.int32))
    return dict(dlogits=final, dlb=dlb, kl_frame=kl_frame, kl_clip=clip_sum(kl_frame, kc))


def old_rows(case):
    """the float32 dlogits an accumulate 1 run of the case starts from: finite everywhere, of the size of a CTC gradient"""
    g = np.random.default_rng(77000 + int(case["name"][:3]))
    return (0.1 * g.standard_normal((case["B"], case["T"], case["C"]))).astype(np.float32)


def measure_k_host():
    """(worst grad ratio, worst KL ratio) of the unmutated twin at k = 1 over the table, accumulate 0 and 1: K_HOST and K_HOST_KL must not
    be below them"""
    kg = kk = 0.0
    for c in cases():
        t0 = twin(c)
        o = old_rows(c)
        kg = max(kg, compare_grad(c, t0["dlogits"], k=1.0), compare_grad(c, twin(c, old=o)["dlogits"], k=1.0, old=o))
        kk = max(kk, compare_kl(c, t0["kl_frame"], k=1.0))
    return kg, kk
