"""CPU: the host half of the device input pipeline — draw_augmentation makes apply_augmentations' `random` calls exactly, the
ishara_clip_aug table matches the header, and the device classes refuse to run without a GPU."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from ishara_amd import _lib
from ishara_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 2, 5, 9, 10, 11, 12, 13, 20, 30, 63, 64, 65, 100, 200, 383, 384, 385, 700]


def _cases():
    g = np.random.default_rng(11)
    return [(n, int(s)) for n in LENGTHS for s in g.integers(0, 1 << 30, 12)]          # 240 (n, seed) cases


def test_draw_consumes_the_rng_exactly_like_apply_augmentations():
    raised = kept = 0
    for n, seed in _cases():
        clip = np.zeros((n, 124, 3), np.float32)
        r_apply, r_draw = random.Random(seed), random.Random(seed)
        try:
            out = D.apply_augmentations(clip, r_apply)
        except ValueError:
            with pytest.raises(ValueError):
                D.draw_augmentation(n, r_draw)
            raised += 1
        else:
            d = D.draw_augmentation(n, r_draw)
            assert d.L2 == out.shape[0], (n, seed, d)
            assert d.n == n and len(d.windows) == len(d.fingers) <= 3
            assert d.L2 == (0 if d.shift == 0 else d.L1)
            kept += 1
        assert r_apply.getstate() == r_draw.getstate(), (n, seed)
    assert kept >= 200 and raised > 0


def test_draw_raises_exactly_where_apply_augmentations_raises():
    for n, seed in _cases():
        try:
            D.apply_augmentations(np.zeros((n, 124, 3), np.float32), random.Random(seed))
            ref = None
        except ValueError:
            ref = ValueError
        try:
            D.draw_augmentation(n, random.Random(seed))
            got = None
        except ValueError:
            got = ValueError
        assert got is ref, (n, seed)


def test_draw_parameters_reproduce_the_augmented_clip():
    """The record alone rebuilds apply_augmentations' output (stretch, shift, mirror, dropout) — what the kernel computes."""
    g = np.random.default_rng(5)
    for n, seed in _cases()[::3]:
        clip = g.standard_normal((n, 124, 3)).astype(np.float32)
        try:
            want = D.apply_augmentations(clip, random.Random(seed))
        except ValueError:
            continue
        d = D.draw_augmentation(n, random.Random(seed))
        got = np.zeros((d.L2, 124, 3), np.float32)
        for j in range(d.L2):
            k = j + (d.shift or 0)
            if not 0 <= k < d.L1:
                continue
            src = 0 if d.L1 == 1 else (n - 1 if k == d.L1 - 1 else int(k * ((n - 1) / (d.L1 - 1))))
            got[j] = clip[src][D._HAND_SWAP] if d.mirror else clip[src]
            if d.mirror:
                got[j, :, 0] = -got[j, :, 0]
            for (t0, t1), m in zip(d.windows, d.fingers):
                if t0 <= j < t1:
                    f = [i for i in range(21) if m >> i & 1]
                    got[j, [76 + i for i in f] + [97 + i for i in f]] = 0
        np.testing.assert_array_equal(got, want)


def test_clip_aug_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    body = re.search(r"typedef struct ishara_clip_aug \{(.*?)\} ishara_clip_aug;", hdr, re.S).group(1)
    fields = re.findall(r"(int64_t|int32_t)\s+([A-Za-z0-9_]+)(?:\[(\d+)\])?;", body)
    ct = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [f[1] for f in fields] == [f[0] for f in _lib.ClipAug._fields_]
    for (ty, name, count), (fname, ftype) in zip(fields, _lib.ClipAug._fields_):
        want = ct[ty] * int(count) if count else ct[ty]
        assert C.sizeof(ftype) == C.sizeof(want) and getattr(ftype, "_type_", ftype) == getattr(want, "_type_", want), name
    assert C.sizeof(_lib.ClipAug) == 64 == D.CLIP_AUG_DTYPE.itemsize
    assert re.search(r"ISHARA_LAYOUT_FLAT = 0, ISHARA_LAYOUT_HANDS_LIPS_XY = 1", hdr)
    assert (_lib.LAYOUT_FLAT, _lib.LAYOUT_HANDS_LIPS_XY) == (0, 1)


def test_fill_clip_table_rows():
    draws = [D.no_augmentation(7), D.AugmentationDraw(40, 44, -3, 44, 1, ((2, 9), (30, 36), (0, 5)), (0b101, 1 << 20, 6)),
             D.AugmentationDraw(30, 24, 0, 0, 0, (), ())]
    tab = np.zeros(3, D.CLIP_AUG_DTYPE)
    D.fill_clip_table(tab, np.array([0, 7, 1 << 33]), draws)
    raw = (_lib.ClipAug * 3).from_buffer_copy(tab.tobytes())
    assert (raw[0].offset, raw[0].n, raw[0].L1, raw[0].shift, raw[0].L2, raw[0].mirror, list(raw[0].fingers)) == (0, 7, 7, 0, 7, 0, [0, 0, 0])
    assert (raw[1].offset, raw[1].L1, raw[1].shift, raw[1].mirror) == (7, 44, -3, 1)
    assert list(raw[1].t0) == [2, 30, 0] and list(raw[1].t1) == [9, 36, 5] and list(raw[1].fingers) == [5, 1 << 20, 6]
    assert (raw[2].offset, raw[2].L1, raw[2].L2) == (1 << 33, 24, 0)


def test_device_pipeline_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.IsharaError):
        D.DeviceClipStore([(np.zeros((3, 124, 3), np.float32), [1])])
    with pytest.raises(_lib.IsharaError):
        D.DeviceBatchAdapter(object(), batch_size=4, T=32)
