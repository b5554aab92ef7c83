"""GPU: ishara_clip_batch (csrc/input_batch.hip) through DeviceClipStore / DeviceBatchAdapter against the host path of
ishara_amd/data.py (apply_augmentations -> pad_resize_normalize -> to_features) and the reference-run fixture."""
import os
import random

import numpy as np
import pytest
import torch

from ishara_amd import _lib, get_model
from ishara_amd import data as D

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "dataloader_adapter.npz")
DEV = "cuda:0"
LENGTHS = [0, 1, 5, 12, 63, 383, 384, 385, 700]
TOL = dict(rtol=1e-7, atol=1e-6)          # rtol: one f32 ulp where short clips normalise to |x| >> 1


def _host(clip, T, layout, rng=None):
    lm = np.asarray(clip, np.float32)
    if rng is not None:
        lm = D.apply_augmentations(lm, rng)
    return D.to_features(D.pad_resize_normalize(lm, T), layout)


def _kernel(store, draws, T, layout, clip_ids=None):
    """ishara_clip_batch on an explicit table (one row per draw, clip i of the store unless clip_ids says otherwise)."""
    ids = np.arange(len(draws)) if clip_ids is None else np.asarray(clip_ids)
    tab = np.zeros(len(draws), D.CLIP_AUG_DTYPE)
    D.fill_clip_table(tab, store.offsets[ids], draws)
    dtab = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    F = 372 if layout == "flat" else 224
    x = torch.full((len(draws), T, F), float("nan"), device=DEV)
    lib = _lib.load()
    _lib.check(lib.ishara_clip_batch(_lib.ptr(store.raw), _lib.ptr(dtab), len(draws), T, {"flat": 0, "hands_lips_xy": 1}[layout],
                                     _lib.ptr(x), None), "ishara_clip_batch")
    torch.cuda.synchronize()
    return x.cpu().numpy()


class _Scripted:
    """An rng that replays the draws of a given AugmentationDraw to apply_augmentations (the host oracle of a forced table)."""

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

    def _pop(self):
        return self.q.pop(0)

    def random(self): return self._pop()
    def uniform(self, a, b): return self._pop()
    def randint(self, a, b): return self._pop()


def _forced(n):
    """Parameter tables covering every branch for a clip of n frames: stretch up / down, shift -10 / +10 / 0, mirror, three
    dropout windows running past L2."""
    out = [D.no_augmentation(n)]
    up, down = max(int(n * 1.19), 1) if n else 0, int(n * 0.81)
    for L1 in {up, down}:
        out.append(D.AugmentationDraw(n, L1, None, L1, 0, (), ()))
    for s in (-10, 10):
        out.append(D.AugmentationDraw(n, up, s, up, 1, (), ()))
        out.append(D.AugmentationDraw(n, down, s, down, 0, (), ()))
    out.append(D.AugmentationDraw(n, n, 0, 0, 1, (), ()))
    L2 = n
    if L2 >= 10:
        wins = ((0, 10), (L2 // 2, L2 // 2 + 7), (L2 - 4, L2 + 6))            # the last one runs past L2
        out.append(D.AugmentationDraw(n, n, None, L2, 1, wins, (0b11, 1 << 20 | 1 << 7, 0x1FFFFF)))
        out.append(D.AugmentationDraw(n, up, -3, up, 0, tuple((t, t + 9) for t in [max(up - 10, 0), 1, 0]), (5, 6, 1 << 12)))
    return out


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def ragged():
    g = np.random.default_rng(3)
    clips = [(g.standard_normal((n, 124, 3)).astype(np.float32) + g.uniform(-1, 1, 3).astype(np.float32), [n % 59, 1])
             for n in LENGTHS]
    return clips, D.DeviceClipStore(clips, DEV)


def test_unaugmented_matches_reference_getitem(gold):
    for ci in range(4):
        lm = gold[f"aug_in_{ci}"]
        T = int(gold[f"item_maxframes_{ci}"])
        store = D.DeviceClipStore([(lm, [1])], DEV)
        got = _kernel(store, [D.no_augmentation(lm.shape[0])], T, "flat")[0]
        np.testing.assert_allclose(got, D.to_features(gold[f"item_x_{ci}"], "flat"), rtol=0, atol=2e-6)


@pytest.mark.parametrize("ci", [0, 3])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_reference_draws_match_the_reference_augmentations(gold, ci, seed):
    lm = gold[f"aug_in_{ci}"]
    T = int(gold[f"item_maxframes_{ci}"])
    store = D.DeviceClipStore([(lm, [1])], DEV)
    d = D.draw_augmentation(lm.shape[0], random.Random(100 * ci + seed))
    got = _kernel(store, [d], T, "flat")[0]
    want = D.to_features(D.pad_resize_normalize(gold[f"aug_out_{ci}_{seed}"], T), "flat")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


def test_scripted_rng_replays_forced_tables():
    g = np.random.default_rng(0)
    for n in (12, 63, 385):
        clip = g.standard_normal((n, 124, 3)).astype(np.float32)
        for d in _forced(n):
            rng = _Scripted(d)
            D.apply_augmentations(clip, rng)
            assert rng.q == [], d


@pytest.mark.parametrize("layout", ["flat", "hands_lips_xy"])
@pytest.mark.parametrize("T", [32, 384])
def test_forced_tables_match_host_path(ragged, layout, T):
    clips, store = ragged
    draws, ids, want = [], [], []
    for ci, (lm, _) in enumerate(clips):
        for d in _forced(lm.shape[0]):
            draws.append(d)
            ids.append(ci)
            want.append(_host(lm, T, layout, _Scripted(d)))
    got = _kernel(store, draws, T, layout, ids)
    for i, w in enumerate(want):
        np.testing.assert_allclose(got[i], w, err_msg=f"clip n={draws[i].n} draw {draws[i]}", **TOL)


def _safe_seed(lengths, start=0):
    """First seed whose draws over `lengths` (in order) raise nowhere."""
    for seed in range(start, start + 1000):
        r = random.Random(seed)
        try:
            for n in lengths:
                D.draw_augmentation(int(n), r)
        except ValueError:
            continue
        return seed
    raise AssertionError("no seed without an empty-clip draw")


def test_seeded_batch_matches_batch_adapter():
    g = np.random.default_rng(8)
    B, T = 256, 384
    lengths = g.integers(12, 701, B)
    lengths[:4] = [12, 384, 385, 700]
    clips = [(g.standard_normal((int(n), 124, 3)).astype(np.float32), [int(i) % 59]) for i, n in enumerate(lengths)]
    seed = _safe_seed(lengths)
    store = D.DeviceClipStore(clips, DEV)
    dev = D.DeviceBatchAdapter(store, B, T, layout="hands_lips_xy", rng=random.Random(seed))
    host = D.BatchAdapter(D.ClipDataset(clips, T, augment=True, rng=random.Random(seed)), B, layout="hands_lips_xy")
    (x, y), = list(dev)
    (xh, yh), = list(host)
    np.testing.assert_array_equal(y.cpu().numpy(), yh)
    np.testing.assert_allclose(x.cpu().numpy(), xh, **TOL)


@pytest.mark.parametrize("layout", ["flat", "hands_lips_xy"])
def test_unaugmented_ragged_batch_matches_host_path(ragged, layout):
    clips, store = ragged
    for T in (32, 384):
        (x, y), = list(D.DeviceBatchAdapter(store, len(clips), T, layout=layout, augment=False))
        xh, yh = D.collate([(D.pad_resize_normalize(lm, T), p) for lm, p in clips], layout)
        np.testing.assert_array_equal(y.cpu().numpy(), yh)
        np.testing.assert_allclose(x.cpu().numpy(), xh, **TOL)
        assert np.all(x[0].cpu().numpy() == 0)                    # n == 0: all zero (std 0)


def test_runs_are_bit_identical(ragged):
    clips, store = ragged
    draws = [d for lm, _ in clips for d in _forced(lm.shape[0])[:4]]
    ids = [ci for ci, (lm, _) in enumerate(clips) for _ in _forced(lm.shape[0])[:4]]
    a = _kernel(store, draws, 384, "hands_lips_xy", ids)
    b = _kernel(store, draws, 384, "hands_lips_xy", ids)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_adapter_order_shuffle_and_shards_follow_batch_adapter():
    g = np.random.default_rng(4)
    clips = [(g.standard_normal((int(n), 124, 3)).astype(np.float32), [i]) for i, n in enumerate(g.integers(20, 90, 10))]
    store = D.DeviceClipStore(clips, DEV, chunk_bytes=1 << 16)                 # several upload chunks
    assert store.n_frames == sum(c[0].shape[0] for c in clips)
    dev = D.DeviceBatchAdapter(store, 4, 32, augment=False, shuffle=True, seed=3)
    host = D.BatchAdapter(D.ClipDataset(clips, 32), 4, shuffle=True, seed=3, layout="hands_lips_xy")
    assert len(dev) == len(host) == 3
    for _ in range(2):                                                          # re-iterable, reshuffled per epoch, same order
        for (x, y), (xh, yh) in zip(dev, host):
            np.testing.assert_array_equal(y.cpu().numpy(), yh)
            np.testing.assert_allclose(x.cpu().numpy(), xh, **TOL)
    seed = _safe_seed([c[0].shape[0] for c in clips[:8]])
    full = D.DeviceBatchAdapter(store, 8, 32, rng=random.Random(seed), drop_last=True)
    (xf, yf), = list(full)
    for rank in range(2):
        sh = D.DeviceBatchAdapter(store, 8, 32, rng=random.Random(seed), drop_last=True, shard=(rank, 2))
        (xs, ys), = list(sh)
        assert torch.equal(xs, xf[4 * rank:4 * rank + 4]) and torch.equal(ys, yf[4 * rank:4 * rank + 4])


def test_rejects_bad_arguments(ragged):
    _, store = ragged
    lib = _lib.load()
    tab = torch.zeros(64, dtype=torch.uint8, device=DEV)
    x = torch.empty(1 * 32 * 224, device=DEV)
    assert lib.ishara_clip_batch(_lib.ptr(store.raw), _lib.ptr(tab), 1, 32, 2, _lib.ptr(x), None) != 0
    assert lib.ishara_clip_batch(_lib.ptr(store.raw), _lib.ptr(tab), 1, 0, 1, _lib.ptr(x), None) != 0
    assert lib.ishara_clip_batch(_lib.ptr(store.raw), _lib.ptr(tab), 1, 5000, 1, _lib.ptr(x), None) != 0
    with pytest.raises(ValueError):
        D.DeviceBatchAdapter(store, 4, 32, layout="xyz")


def test_model_on_device_batches():
    g = np.random.default_rng(6)
    B, T = 8, 64
    clips = [(g.standard_normal((int(n), 124, 3)).astype(np.float32), list(g.integers(0, 59, 6)))
             for n in g.integers(30, 120, 3 * B)]
    seed = _safe_seed([c[0].shape[0] for c in clips])
    store = D.DeviceClipStore(clips, DEV)
    dev = D.DeviceBatchAdapter(store, B, T, rng=random.Random(seed))
    host = D.BatchAdapter(D.ClipDataset(clips, T, augment=True, rng=random.Random(seed)), B, layout="hands_lips_xy")
    model = get_model(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(T, 224), dtype="f32",
                      max_batch=B, device=DEV, seed=0)
    (x, y), (xh, yh) = next(iter(dev)), next(iter(host))
    np.testing.assert_array_equal(y.cpu().numpy(), yh)
    la = model(x, training=False).cpu().numpy()
    lb = model(xh, training=False).cpu().numpy()
    assert np.abs(la - lb).max() < 1e-4
    hist = model.fit(D.DeviceBatchAdapter(store, B, T, rng=random.Random(seed)), epochs=1, verbose=0)
    assert np.isfinite(hist.history["loss"][0])
