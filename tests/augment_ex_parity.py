"""The cases and the host composition shared by tests/test_augment_ex_gpu.py (ishara_clip_batch_ex against them) and
tests/test_augment_ex_mutants.py (ordinary mistakes applied to the same composition on the same cases).

A case is (clip index, AugmentationDrawEx): every branch of the existing forced draws (stretch up / down, shift +-10 and the emptying 0,
mirror, three dropout windows with one running past L2) x three affines x five masks, on clips of n in LENGTHS frames at T in TS."""
import numpy as np

from ishara_amd import data as D

LENGTHS = [0, 1, 12, 63, 385]
TS = [32, 64]
LAYOUTS = ["flat", "hands_lips_xy"]
TOL = dict(rtol=1e-7, atol=1e-6)          # the tolerance of tests/test_input_pipeline_gpu.py

# (scale, shear_x, shear_y, degree, shift): the identity and the two corners of the reference's ranges
AFFINES = [None, (1.2, 0.15, 0.0, 30.0, 0.1), (0.8, 0.0, -0.15, -30.0, -0.1)]


class Scripted:
    """An rng that replays the draws of an AugmentationDraw to apply_augmentations (the host oracle of a forced table)."""

    def __init__(self, d):
        q = []
        q += [0.0, (d.L1 + 0.5) / d.n] if d.L1 != d.n else [0.99]
        q += [0.0, d.shift] if d.shift is not None else [0.99]
        q += [0.0] if d.mirror else [0.99]
        if d.windows:
            fs = [[i for i in range(21) if m >> i & 1] for m in d.fingers]
            nf = max(len(f) for f in fs)                       # one finger count for all windows; repeats collapse
            q += [0.0, nf, len(d.windows)]
            for (t0, t1), f in zip(d.windows, fs):
                q += [t0, t1 - t0] + f + [f[-1]] * (nf - len(f))
        else:
            q += [0.99]
        self.q = q

    def random(self): return self.q.pop(0)
    def uniform(self, a, b): return self.q.pop(0)
    def randint(self, a, b): return self.q.pop(0)


def clips():
    """The raw clips: gaussian landmarks off centre (so that a zero frame is far from the mean), one per length."""
    g = np.random.default_rng(17)
    return [(g.standard_normal((n, 124, 3)).astype(np.float32) + g.uniform(-1, 1, 3).astype(np.float32), [n % 59, 1]) for n in LENGTHS]


def base_draws(n):
    """Every branch of draw_augmentation for a clip of n frames."""
    out = [D.no_augmentation(n)]
    up, down = max(int(n * 1.19), 1) if n else 0, int(n * 0.81)
    out.append(D.AugmentationDraw(n, up, None, up, 0, (), ()))
    out.append(D.AugmentationDraw(n, down, 10, down, 1, (), ()))
    out.append(D.AugmentationDraw(n, up, -10, up, 0, (), ()))
    out.append(D.AugmentationDraw(n, n, 0, 0, 1, (), ()))                         # a drawn shift of 0 empties the clip
    if n >= 10:
        wins = ((0, 10), (n // 2, n // 2 + 7), (n - 4, n + 6))                    # the last one runs past L2
        out.append(D.AugmentationDraw(n, n, None, n, 1, wins, (0b11, 1 << 20 | 1 << 7, 0x1FFFFF)))
        out.append(D.AugmentationDraw(n, up, -3, up, 0, tuple((t, t + 9) for t in [max(up - 10, 0), 1, 0]), (5, 6, 1 << 12)))
    return out


def masks(L2):
    """none, interior, starting at 0, ending at L2, the whole clip (those that differ at this L2)"""
    k = max(L2 // 3, 1)
    out = [(0, 0)]
    for m in [(L2 // 3, L2 // 3 + max(L2 // 4, 1)), (0, k), (L2 - k, L2), (0, L2)]:
        if 0 <= m[0] < m[1] <= L2 and m not in out:
            out.append(m)
    return out


def affine(spec):
    if spec is None:
        return (1.0, 0.0, 0.0, 1.0), 0.0
    scale, shx, shy, deg, shift = spec
    return D.affine_matrix(scale, shx, shy, deg), float(np.float32(shift))


def cases():
    """[(clip index, AugmentationDrawEx)]"""
    out = []
    for ci, n in enumerate(LENGTHS):
        for d in base_draws(n):
            for spec in AFFINES:
                M, shift = affine(spec)
                for m0, m1 in masks(d.L2):
                    out.append((ci, D.AugmentationDrawEx(d, M, shift, m0, m1)))
    return out


def frame_len(d, T):
    return min(d.draw.L2, T) if d.draw.n > 0 else 0


def host(clip, d, T, mut=None):
    """The host composition of one case -> [T,124,3] float32: affine_xy on the raw clip, apply_augmentations on the scripted draws, the
    mask, pad_resize_normalize.  `mut` names one ordinary mistake (tests/test_augment_ex_mutants.py)."""
    lm = np.asarray(clip, np.float32)
    M, shift = d.M, d.shift
    if mut == "M_transposed":
        M = (M[0], M[2], M[1], M[3])
    if mut == "scale_dropped":
        s = np.sqrt(np.float64(M[0]) * M[3] - np.float64(M[1]) * M[2])        # det(M) = scale^2 (1 - shear_x shear_y), one shear is 0
        M = tuple(float(np.float32(v / s)) for v in M)
    if mut == "shift_dropped":
        shift = 0.0

    def aff(c):
        c = D.affine_xy(c, M, shift)
        if mut == "shift_on_z":
            c[..., 2] = (c[..., 2].astype(np.float64) + np.float64(np.float32(shift))).astype(np.float32)
        return c

    if mut == "affine_after_mirror":
        lm = aff(D.apply_augmentations(lm, Scripted(d.draw)))
    else:
        lm = D.apply_augmentations(aff(lm), Scripted(d.draw))
    if mut == "shift_on_zero_frames":                          # the affine applied to the augmented clip's zero frames as well
        zero = ~lm.any(axis=(1, 2))
        lm[zero, :, :2] += np.float32(shift)
    m0, m1 = d.m0, d.m1
    if mut == "mask_one_short" and m1 > m0:
        m1 -= 1
    if mut == "mask_one_late" and m1 > m0:
        m0, m1 = m0 + 1, m1 + 1
    lm = lm.copy()
    lm[m0:m1] = 0
    if mut == "shift_on_zero_frames" and m1 > m0:
        lm[m0:m1, :, :2] += np.float32(shift)
    out = D.pad_resize_normalize(lm, T)
    if mut == "shift_on_zero_frames" and lm.shape[0] < T:      # ... and to the padding
        padded = np.zeros((T, 124, 3), np.float64)
        padded[:lm.shape[0]] = lm
        padded[lm.shape[0]:, :, :2] += np.float32(shift)
        mu, sd = padded.mean(axis=(0, 1), keepdims=True), padded.std(axis=(0, 1), keepdims=True)
        out = ((padded - mu) / (sd + 1e-8)).astype(np.float32)
    return out


_ref = {}


def reference(T):
    """The host composition of every case at T, computed once: [n_cases, T, 124, 3] float32"""
    if T not in _ref:
        cl = clips()
        ref = np.stack([host(cl[ci][0], d, T) for ci, d in cases()])
        ref.setflags(write=False)
        _ref[T] = ref
    return _ref[T]
