"""CPU: the host reference of the spatial affine and the temporal mask (ishara_amd/data.py *_ex): the rng call sequence, the table row,
the affine's values and the mask's bounds.  The kernel is held to this reference in tests/test_augment_ex_gpu.py."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from ishara_amd import _lib
from ishara_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 9, 10, 12, 63, 384, 385, 700]


def _draw(fn, *a, **kw):
    """fn's result, or the ValueError it raises (a dropout window on a clip shorter than 10 frames)"""
    try:
        return fn(*a, **kw)
    except ValueError:
        return "ValueError"


def test_both_options_off_is_draw_augmentation():
    for seed in range(200):
        for n in LENGTHS:
            a, b = random.Random(seed), random.Random(seed)
            want, got = _draw(D.draw_augmentation, n, a), _draw(D.draw_augmentation_ex, n, b)
            assert a.getstate() == b.getstate(), (seed, n)
            if want == "ValueError":
                assert got == "ValueError"
                continue
            assert got == D.AugmentationDrawEx(want, (1.0, 0.0, 0.0, 1.0), 0.0, 0, 0), (seed, n)
    r = random.Random(5)
    state = r.getstate()
    assert D.draw_augmentation_ex(40, r, augment=False) == D.no_augmentation_ex(40) and r.getstate() == state


@pytest.mark.parametrize("opts", [dict(spatial_affine=True), dict(temporal_mask=True), dict(spatial_affine=True, temporal_mask=True),
                                  dict(augment=False, spatial_affine=True, temporal_mask=True),
                                  dict(spatial_affine=D.AffineRanges(scale=(0.5, 2.0), p=1.0), temporal_mask=D.MaskRanges((0.0, 1.0), 1.0))],
                         ids=["affine", "mask", "both", "both_only", "ranges"])
def test_apply_and_draw_consume_the_same_draws(opts):
    g = np.random.default_rng(0)
    for seed in range(60):
        for n in (0, 1, 12, 63, 385):
            clip = g.standard_normal((n, 124, 3)).astype(np.float32)
            a, b = random.Random(seed), random.Random(seed)
            d, out = _draw(D.draw_augmentation_ex, n, a, **opts), _draw(D.apply_augmentations_ex, clip, b, **opts)
            assert a.getstate() == b.getstate(), (seed, n)
            if isinstance(d, str):
                assert isinstance(out, str)
                continue
            assert out.shape[0] == d.draw.L2 and out.dtype == np.float32
            assert 0 <= d.m0 <= d.m1 <= d.draw.L2
            assert not out[d.m0:d.m1].any()


def test_apply_equals_the_composition_of_its_draw():
    """apply_augmentations_ex = affine_xy -> apply_augmentations -> mask, on the parameters draw_augmentation_ex reports"""
    g = np.random.default_rng(1)
    clip = g.standard_normal((63, 124, 3)).astype(np.float32)
    n_aff = n_mask = 0
    for seed in range(40):
        d = D.draw_augmentation_ex(63, random.Random(seed), spatial_affine=True, temporal_mask=True)
        got = D.apply_augmentations_ex(clip, random.Random(seed), spatial_affine=True, temporal_mask=True)
        r = random.Random(seed)
        D._draw_affine(r, D.AffineRanges())                # past the affine block: the existing draws come next
        want = D.apply_augmentations(D.affine_xy(clip, d.M, d.shift), r)
        want[d.m0:d.m1] = 0
        assert np.array_equal(got, want)
        n_aff += d.M != (1.0, 0.0, 0.0, 1.0)
        n_mask += d.m1 > d.m0
    assert 20 <= n_aff < 40 and 10 <= n_mask < 35          # both gates fire and fail (p = 0.75, 0.5)


def test_draw_order_and_the_coin():
    class Log:
        def __init__(self, vals): self.vals, self.calls = list(vals), []
        def random(self): self.calls.append("random"); return self.vals.pop(0)
        def uniform(self, a, b): self.calls.append(("uniform", a, b)); return self.vals.pop(0)
        def randrange(self, n): self.calls.append(("randrange", n)); return self.vals.pop(0)
        def randint(self, a, b): self.calls.append(("randint", a, b)); return self.vals.pop(0)

    #            gate scale shear coin deg   shift | the four gates of draw_augmentation | gate frac offset
    r = Log([0.7, 1.1, 0.1, 0.4, 20.0, 0.05, 0.9, 0.9, 0.9, 0.9, 0.4, 0.25, 7])
    d = D.draw_augmentation_ex(100, r, spatial_affine=True, temporal_mask=True)
    assert r.calls == ["random", ("uniform", 0.8, 1.2), ("uniform", -0.15, 0.15), "random", ("uniform", -30, 30), ("uniform", -0.1, 0.1),
                       "random", "random", "random", "random", "random", ("uniform", 0.2, 0.4), ("randrange", 75)]
    assert (d.m0, d.m1) == (7, 32) and d.draw == D.no_augmentation(100)
    assert d.M == D.affine_matrix(1.1, 0.0, 0.1, 20.0) and d.shift == float(np.float32(0.05))         # coin < 0.5: shear_y
    r = Log([0.7, 1.1, 0.1, 0.5, 20.0, 0.05, 0.6])
    d = D.draw_augmentation_ex(100, r, augment=False, spatial_affine=True, temporal_mask=True)
    assert d.M == D.affine_matrix(1.1, 0.1, 0.0, 20.0) and (d.m0, d.m1) == (0, 0) and r.vals == []      # coin >= 0.5: shear_x
    r = Log([0.75, 0.5])                                                                               # both gates fail at p
    assert D.draw_augmentation_ex(100, r, augment=False, spatial_affine=True, temporal_mask=True) == D.no_augmentation_ex(100)
    r = Log([0.0, 0.3])                                                                                # L2 == 0 draws no offset
    d = D.draw_augmentation_ex(0, r, augment=False, temporal_mask=True)
    assert (d.m0, d.m1) == (0, 0) and r.calls == ["random", ("uniform", 0.2, 0.4)]
    r = Log([0.0, 0.2, 0])                                                                             # size 0 on a short clip
    d = D.draw_augmentation_ex(3, r, augment=False, temporal_mask=True)
    assert (d.m0, d.m1) == (0, 0) and r.calls[-1] == ("randrange", 3)


def test_mask_bounds():
    for seed in range(200):
        r = random.Random(seed)
        for n in LENGTHS:
            d = _draw(D.draw_augmentation_ex, n, r, temporal_mask=D.MaskRanges(p=1.0))
            if isinstance(d, str):
                continue
            L2 = d.draw.L2
            assert 0 <= d.m0 <= d.m1 <= L2 and int(L2 * 0.2) <= d.m1 - d.m0 <= int(L2 * 0.4)


def test_clip_aug_ex_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    body = re.search(r"typedef struct ishara_clip_aug_ex \{(.*?)\} ishara_clip_aug_ex;", hdr, re.S).group(1)
    fields = re.findall(r"(int64_t|int32_t|float|ishara_clip_aug)\s+([a-z_0-9, ]+?)(?:\[(\d+)\])?;", body)
    names = [n.strip() for _, group, _ in fields for n in group.split(",")]
    assert names == [f[0] for f in _lib.ClipAugEx._fields_]
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "ishara_clip_aug": _lib.ClipAug}
    want = [ctype[ty] * int(cnt) if cnt else ctype[ty] for ty, group, cnt in fields for _ in group.split(",")]
    for w, (fname, ftype) in zip(want, _lib.ClipAugEx._fields_):
        assert w is ftype, fname                            # ctypes caches array types: c_float * 4 is one object
    assert C.sizeof(_lib.ClipAugEx) == 96 == D.CLIP_AUG_EX_DTYPE.itemsize
    assert hdr.index("} ishara_clip_aug;") < hdr.index("typedef struct ishara_clip_aug_ex")
    assert _lib.ClipAugEx.m.offset == 64 and _lib.ClipAugEx.reserved.offset == 92


def test_fill_clip_table_ex_round_trips():
    d = D.AugmentationDrawEx(D.AugmentationDraw(50, 45, -3, 45, 1, ((1, 8), (30, 39)), (0b101, 1 << 20)), (0.5, -0.25, 0.125, 2.0), 0.0625, 4, 17)
    tab = np.zeros(2, D.CLIP_AUG_EX_DTYPE)
    D.fill_clip_table_ex(tab, np.array([7, 1 << 33]), [d, D.no_augmentation_ex(9)])
    raw = (_lib.ClipAugEx * 2).from_buffer_copy(tab.tobytes())
    r = raw[0]
    assert (r.base.offset, r.base.n, r.base.L1, r.base.shift, r.base.L2, r.base.mirror) == (7, 50, 45, -3, 45, 1)
    assert list(r.base.t0) == [1, 30, 0] and list(r.base.t1) == [8, 39, 0] and list(r.base.fingers) == [0b101, 1 << 20, 0]
    assert list(r.m) == [0.5, -0.25, 0.125, 2.0] and r.shift_xy == 0.0625 and (r.m0, r.m1, r.reserved) == (4, 17, 0)
    r = raw[1]
    assert (r.base.offset, r.base.n, r.base.L2) == (1 << 33, 9, 9) and list(r.m) == [1.0, 0.0, 0.0, 1.0] and (r.shift_xy, r.m0, r.m1) == (0.0, 0, 0)
    old = np.zeros(2, D.CLIP_AUG_DTYPE)
    D.fill_clip_table(old, np.array([7, 1 << 33]), [d.draw, D.no_augmentation(9)])
    assert tab["base"].tobytes() == old.tobytes()


def test_identity_affine_without_mask_is_apply_augmentations():
    g = np.random.default_rng(2)
    never = D.AffineRanges(p=0.0)                           # the gate is drawn and fails: the identity is applied
    for seed in range(30):
        for n in (12, 63, 385):
            clip = g.standard_normal((n, 124, 3)).astype(np.float32)
            r = random.Random(seed)
            r.random()
            want = _draw(D.apply_augmentations, clip, r)
            got = _draw(D.apply_augmentations_ex, clip, random.Random(seed), spatial_affine=never)
            if isinstance(want, str):
                assert isinstance(got, str)
                continue
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert D.affine_xy(clip, (1.0, 0.0, 0.0, 1.0), 0.0).tobytes() == clip.tobytes()


def test_affine_agrees_with_the_sequential_restatement():
    """scale -> shear -> rotate -> shift in fp64, one step after the other as the reference applies them, against the composed float32 M:
    rounding M and shift to float32 and the output rounding cost at most 2^-23 * 1.4 * (|x| + |y| + 1) (|M| entries <= 1.2 * 1.15); the
    bound applied is 2^-21 * (|x| + |y| + 1)."""
    g = np.random.default_rng(3)
    clip = (g.standard_normal((40, 124, 3)) * g.uniform(0.1, 4.0)).astype(np.float32)
    x, y = clip[..., 0].astype(np.float64), clip[..., 1].astype(np.float64)
    bound = 2.0 ** -21 * (np.abs(x) + np.abs(y) + 1.0)
    worst = 0.0
    for seed in range(50):
        r = random.Random(seed)
        scale, sh, coin, deg, shift = r.uniform(0.8, 1.2), r.uniform(-0.15, 0.15), r.random(), r.uniform(-30, 30), r.uniform(-0.1, 0.1)
        shx, shy = (0.0, sh) if coin < 0.5 else (sh, 0.0)
        xy = np.stack([x, y], -1) * scale
        xy = xy @ np.array([[1.0, shx], [shy, 1.0]])
        a = deg * np.pi / 180
        xy = xy @ np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        xy = xy + shift
        got = D.affine_xy(clip, D.affine_matrix(scale, shx, shy, deg), np.float32(shift))
        assert got.dtype == np.float32 and np.array_equal(got[..., 2], clip[..., 2])
        err = np.abs(got[..., :2].astype(np.float64) - xy)
        worst = max(worst, float((err / bound[..., None]).max()))
        assert (err <= bound[..., None]).all(), seed
    print(f"worst error / bound: {worst:.3f}")


def test_clip_dataset_twin_and_option_forms():
    g = np.random.default_rng(4)
    clips = [(g.standard_normal((n, 124, 3)).astype(np.float32), [1]) for n in (40, 90)]
    ds = D.ClipDataset(clips, 32, augment=True, rng=random.Random(9), spatial_affine=True, temporal_mask=D.MaskRanges())
    r = random.Random(9)
    for i in range(2):
        want = D.pad_resize_normalize(D.apply_augmentations_ex(clips[i][0], r, True, D.AffineRanges(), True), 32)
        assert np.array_equal(ds[i][0], want)
    a = D.ClipDataset(clips, 32, augment=True, rng=random.Random(9))
    r = random.Random(9)
    assert np.array_equal(a[0][0], D.pad_resize_normalize(D.apply_augmentations(clips[0][0], r), 32))
