"""Batch adapter for the reference's torch loader contract.

`data_loader.py`'s `ASLDataset.__getitem__` yields `(landmarks float32 [max_frames, 124, 3], List[int])`
(data_loader.py:166-195) and its DataLoader has no collate for the ragged phrases.  This module restates the
host-side steps of that file — augmentations (`:129-166`, same `random` call sequence, so a seeded
`random.Random` reproduces the reference's draws), pad / resize to `max_frames` (`:176-185`), per-sample
normalisation (`:187-188`) — and adds the collate the encoder needs: x `[B, T, F]` float32 with
F = 124*3 (flattened) or 112*2 (hands + lips x,y only: the F=224 of BASELINE config #2), y `[B, 64]` int64
padded with 59 (conv-hybrid-model.ipynb c4:21-23)."""
from __future__ import annotations

import math
import random
from typing import Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ._lib import ClipAug, ClipAugEx

MAX_PHRASE_LENGTH = 64   # c1:33
PAD_TOKEN_IDX = 59       # c1:5
N_FACE, N_HAND, N_POSE = 76, 21, 6          # data_loader.py:66-71 (face, left hand, right hand, pose) = 124 landmarks
LEFT_START, RIGHT_START = N_FACE, N_FACE + N_HAND


_HAND_SWAP = np.arange(N_FACE + 2 * N_HAND + N_POSE)
_HAND_SWAP[LEFT_START:LEFT_START + N_HAND] = np.arange(RIGHT_START, RIGHT_START + N_HAND)
_HAND_SWAP[RIGHT_START:RIGHT_START + N_HAND] = np.arange(LEFT_START, LEFT_START + N_HAND)


def _resample_time(clip: np.ndarray, length: int) -> np.ndarray:
    """Nearest-below resample along time: frame j of the result is frame floor(j * (T - 1) / (length - 1))."""
    return clip[np.linspace(0, clip.shape[0] - 1, length).astype(np.int64)]


def apply_augmentations(landmarks: np.ndarray, rng: random.Random) -> np.ndarray:
    """The four augmentations of `ASLDataset._apply_augmentations` (data_loader.py:124-166) on one clip `[T,124,3]`,
    drawing from `rng` in the reference's order (gate, then that augmentation's parameters), so a seeded
    `random.Random` reproduces its output.  Returns a new array; the input is not modified."""
    clip = np.array(landmarks)
    if rng.random() < 0.8:                                        # time stretch by 0.8x-1.2x
        clip = _resample_time(clip, int(clip.shape[0] * rng.uniform(0.8, 1.2)))
    if rng.random() < 0.5:                                        # shift by up to 10 frames, zero fill
        s, n = rng.randint(-10, 10), clip.shape[0]
        moved = np.zeros_like(clip)
        if s > 0:
            moved[:max(n - s, 0)] = clip[s:]
        elif s < 0:
            moved[-s:] = clip[:max(n + s, 0)]
        else:
            moved = moved[:0]                                     # the reference's `[:shift]` with shift == 0 is empty
        clip = moved
    if rng.random() < 0.5:                                        # mirror: swap the hands, negate x
        clip = clip[:, _HAND_SWAP]
        clip[..., 0] = -clip[..., 0]
    if rng.random() < 0.5:                                        # finger dropout in 2-3 short windows
        n_fingers, n_windows = rng.randint(2, 6), rng.randint(2, 3)
        for _ in range(n_windows):
            t0 = rng.randint(0, clip.shape[0] - 10)
            t1 = t0 + rng.randint(5, 10)
            fingers = np.array([rng.randint(0, 20) for _ in range(n_fingers)])
            clip[t0:t1, np.concatenate([LEFT_START + fingers, RIGHT_START + fingers])] = 0
    return clip


def pad_resize_normalize(landmarks: np.ndarray, max_frames: int = 384) -> np.ndarray:
    """data_loader.py:176-188: clips longer than `max_frames` are resampled down (nearest-below), shorter ones
    zero-padded at the end; then each coordinate is z-normalised over (frames, landmarks), eps 1e-8 on the std."""
    n = landmarks.shape[0]
    if n > max_frames:
        clip = _resample_time(landmarks, max_frames).astype(np.float64)
    else:
        clip = np.zeros((max_frames,) + landmarks.shape[1:], np.float64)
        clip[:n] = landmarks
    mu, sd = clip.mean(axis=(0, 1), keepdims=True), clip.std(axis=(0, 1), keepdims=True)
    return ((clip - mu) / (sd + 1e-8)).astype(np.float32)


def to_features(landmarks: np.ndarray, layout: str = "flat") -> np.ndarray:
    """[T, 124, 3] -> [T, F].  "flat": all landmarks, xyz (F = 372).  "hands_lips_xy": the two hands + the first 70
    face landmarks, x and y only (F = 112 * 2 = 224, the feature width BASELINE config #2 is quoted on)."""
    if layout == "flat":
        return landmarks.reshape(landmarks.shape[0], -1)
    if layout == "hands_lips_xy":
        sel = np.concatenate([np.arange(LEFT_START, LEFT_START + 2 * N_HAND), np.arange(0, 70)])
        return landmarks[:, sel, :2].reshape(landmarks.shape[0], -1)
    raise ValueError(f"unknown layout {layout!r}")


def pad_phrase(phrase: Sequence[int], max_len: int = MAX_PHRASE_LENGTH, pad: int = PAD_TOKEN_IDX) -> np.ndarray:
    """tf.pad(phrase, [[0, MAX_PHRASE_LENGTH - len]], constant_values=pad_token_idx) — c4:21-22."""
    if len(phrase) > max_len:
        raise ValueError(f"phrase of {len(phrase)} tokens exceeds MAX_PHRASE_LENGTH={max_len}")
    out = np.full(max_len, pad, np.int64)
    out[:len(phrase)] = np.asarray(phrase, np.int64)
    return out


def collate(samples: Iterable[Tuple[np.ndarray, Sequence[int]]], layout: str = "flat") -> Tuple[np.ndarray, np.ndarray]:
    """List of `(landmarks [T,124,3], phrase List[int])` -> `(x [B,T,F] float32, y [B,64] int64)`: the collate the
    reference's DataLoader lacks (its default collate fails on the ragged phrases)."""
    xs, ys = [], []
    for lm, phrase in samples:
        lm = np.asarray(lm.numpy() if hasattr(lm, "numpy") else lm, np.float32)
        xs.append(to_features(lm, layout))
        ys.append(pad_phrase(phrase))
    return np.stack(xs).astype(np.float32), np.stack(ys)


class BatchAdapter:
    """Re-iterable `(x, y)` batch stream over an `ASLDataset`-shaped indexable (anything with `__len__` and
    `__getitem__ -> (landmarks, phrase)`), the `train_dataset` argument of `Model.fit`."""

    def __init__(self, dataset, batch_size: int = 64, shuffle: bool = False, seed: int = 0, layout: str = "flat",
                 drop_last: bool = False, device: Optional[str] = None):
        self.dataset, self.batch_size, self.shuffle, self.layout = dataset, batch_size, shuffle, layout
        self.drop_last, self.device = drop_last, device
        self._rng = np.random.default_rng(seed)

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self) -> Iterator[Tuple["np.ndarray", "np.ndarray"]]:
        order = np.arange(len(self.dataset))
        if self.shuffle:
            self._rng.shuffle(order)
        for i in range(0, len(order), self.batch_size):
            idx = order[i:i + self.batch_size]
            if self.drop_last and len(idx) < self.batch_size:
                break
            x, y = collate([self.dataset[int(j)] for j in idx], self.layout)
            if self.device is not None:
                import torch
                yield torch.from_numpy(x).to(self.device), torch.from_numpy(y).to(self.device)
            else:
                yield x, y


# ---------------------------------------------------------------------------------------------------------------------
# Device-resident input pipeline: the raw clips live on the GPU (DeviceClipStore), the host only draws each clip's
# augmentation parameters (draw_augmentation) into a 64-byte table row, and ONE kernel (ishara_clip_batch, csrc/input_batch.hip)
# builds the normalised, collated batch.  apply_augmentations / pad_resize_normalize / collate / BatchAdapter above stay the
# oracle of this path.

class AugmentationDraw(NamedTuple):
    """The parameters `apply_augmentations` draws for one clip.  `shift` is None when no shift was drawn; `L2 == 0` after a drawn
    shift of 0 (the reference's `[:0]`).  `windows[i] = (t0, t1)` over the augmented frames, `fingers[i]` its 21-bit finger mask."""
    n: int
    L1: int
    shift: Optional[int]
    L2: int
    mirror: int
    windows: Tuple[Tuple[int, int], ...]
    fingers: Tuple[int, ...]


def draw_augmentation(n_frames: int, rng: random.Random) -> AugmentationDraw:
    """Draw what `apply_augmentations` would apply to a clip of `n_frames` frames, making exactly its `rng` calls in its order and
    touching no landmark data; raises ValueError where it raises (a dropout window on a clip shorter than 10 frames)."""
    n = int(n_frames)
    L1, shift, mirror, windows, fingers = n, None, 0, [], []
    if rng.random() < 0.8:
        L1 = int(n * rng.uniform(0.8, 1.2))
    L2 = L1
    if rng.random() < 0.5:
        shift = rng.randint(-10, 10)
        if shift == 0:
            L2 = 0
    if rng.random() < 0.5:
        mirror = 1
    if rng.random() < 0.5:
        n_fingers, n_windows = rng.randint(2, 6), rng.randint(2, 3)
        for _ in range(n_windows):
            t0 = rng.randint(0, L2 - 10)
            t1 = t0 + rng.randint(5, 10)
            mask = 0
            for _ in range(n_fingers):
                mask |= 1 << rng.randint(0, 20)
            windows.append((t0, t1))
            fingers.append(mask)
    return AugmentationDraw(n, L1, shift, L2, mirror, tuple(windows), tuple(fingers))


def no_augmentation(n_frames: int) -> AugmentationDraw:
    n = int(n_frames)
    return AugmentationDraw(n, n, None, n, 0, (), ())


def fill_clip_table(table: np.ndarray, offsets: np.ndarray, draws: Sequence[AugmentationDraw]) -> None:
    """Write one `ishara_clip_aug` row per clip into `table` (a numpy view with the dtype of `_lib.ClipAug`)."""
    b = len(draws)
    table["offset"] = offsets
    table["n"] = [d.n for d in draws]
    table["L1"] = [d.L1 for d in draws]
    table["shift"] = [d.shift or 0 for d in draws]
    table["L2"] = [d.L2 for d in draws]
    table["mirror"] = [d.mirror for d in draws]
    win = np.zeros((b, 3, 3), np.int32)                 # t0, t1, fingers
    for i, d in enumerate(draws):
        for w, ((t0, t1), m) in enumerate(zip(d.windows, d.fingers)):
            win[i, :, w] = (t0, t1, m)
    table["t0"], table["t1"], table["fingers"] = win[:, 0], win[:, 1], win[:, 2]


# ---------------------------------------------------------------------------------------------------------------------
# The two augmentations of the reference's CTC training script (Test Notebooks/asl-translation-nb4.ipynb: spatial_random_affine
# with probability 0.75, temporal_mask with probability 0.5, chained by augment_fn), restated on the `random` draws of this module:
# the affine on the raw clip, then apply_augmentations, then the mask over the augmented frames.  With both off, every function
# below makes exactly the rng calls of its namesake above.  DESIGN §3 (spatial affine, temporal mask and frame counts).

class AffineRanges(NamedTuple):
    """Ranges of `spatial_random_affine` (the reference's defaults) and the probability `augment_fn` applies it with."""
    scale: Tuple[float, float] = (0.8, 1.2)
    shear: Tuple[float, float] = (-0.15, 0.15)
    degree: Tuple[float, float] = (-30, 30)
    shift: Tuple[float, float] = (-0.1, 0.1)
    p: float = 0.75


class MaskRanges(NamedTuple):
    """Range of `temporal_mask`'s size (a fraction of the clip's frames) and the probability `augment_fn` applies it with."""
    size: Tuple[float, float] = (0.2, 0.4)
    p: float = 0.5


class AugmentationDrawEx(NamedTuple):
    """`AugmentationDraw` plus the affine (`M` = (M00, M01, M10, M11) and `shift`, float32 values) and the temporal mask `[m0, m1)`
    over the augmented frames (`m0 == m1`: none)."""
    draw: AugmentationDraw
    M: Tuple[float, float, float, float]
    shift: float
    m0: int
    m1: int


_IDENTITY = (1.0, 0.0, 0.0, 1.0)


def _ranges(option, default):
    """None / False: off; True: the reference's defaults; a ranges tuple: those ranges."""
    if option is None or option is False:
        return None
    return default() if option is True else default(*option)


def affine_matrix(scale: float, shear_x: float, shear_y: float, degree: float) -> Tuple[float, float, float, float]:
    """`M = scale * [[1, shear_x], [shear_y, 1]] @ [[cos, -sin], [sin, cos]]` in fp64, each entry rounded to float32: the scale, shear and
    rotation of `spatial_random_affine` composed for the row-vector convention `[x' y'] = [x y] @ M`."""
    a = float(degree) * math.pi / 180.0
    c, s, k, hx, hy = math.cos(a), math.sin(a), float(scale), float(shear_x), float(shear_y)
    M = (k * (c + hx * s), k * (hx * c - s), k * (hy * c + s), k * (c - hy * s))
    return tuple(float(v) for v in np.array(M, np.float32))


def _draw_affine(rng, r: AffineRanges):
    """The affine block's draws: (M, shift) as float32 values, the identity when the gate fails."""
    if not rng.random() < r.p:
        return _IDENTITY, 0.0
    scale, sh, coin = rng.uniform(*r.scale), rng.uniform(*r.shear), rng.random()
    shear_x, shear_y = (0.0, sh) if coin < 0.5 else (sh, 0.0)           # the reference's coin
    deg, shift = rng.uniform(*r.degree), rng.uniform(*r.shift)
    return affine_matrix(scale, shear_x, shear_y, deg), float(np.float32(shift))


def _draw_mask(rng, r: MaskRanges, L2: int) -> Tuple[int, int]:
    """The mask block's draws over a clip of L2 augmented frames: [m0, m1), (0, 0) when the gate fails."""
    if not rng.random() < r.p:
        return 0, 0
    size = int(L2 * rng.uniform(*r.size))
    m0 = rng.randrange(L2 - size) if L2 > size else 0
    return m0, m0 + size


def affine_xy(landmarks: np.ndarray, M, shift: float) -> np.ndarray:
    """`[x' y'] = [x y] @ M + shift` on a clip `[n,124,3]` of float32 values, z untouched: each product and the sum `(p + q) + shift` in
    fp64, the result rounded to float32.  A product of two float32 values is exact in fp64, so the bits do not depend on FMA contraction."""
    clip = np.array(landmarks, np.float32)
    m00, m01, m10, m11 = (np.float64(np.float32(v)) for v in M)
    s = np.float64(np.float32(shift))
    x, y = clip[..., 0].astype(np.float64), clip[..., 1].astype(np.float64)
    clip[..., 0] = ((m00 * x + m10 * y) + s).astype(np.float32)
    clip[..., 1] = ((m01 * x + m11 * y) + s).astype(np.float32)
    return clip


def draw_augmentation_ex(n_frames: int, rng, augment: bool = True, spatial_affine=None, temporal_mask=None) -> AugmentationDrawEx:
    """Draw what `apply_augmentations_ex` would apply to a clip of `n_frames` frames, making exactly its `rng` calls in its order: the
    affine block (if on), `draw_augmentation` (if `augment`), the mask block (if on)."""
    aff, msk = _ranges(spatial_affine, AffineRanges), _ranges(temporal_mask, MaskRanges)
    M, shift = _draw_affine(rng, aff) if aff is not None else (_IDENTITY, 0.0)
    d = draw_augmentation(n_frames, rng) if augment else no_augmentation(n_frames)
    m0, m1 = _draw_mask(rng, msk, d.L2) if msk is not None else (0, 0)
    return AugmentationDrawEx(d, M, shift, m0, m1)


def apply_augmentations_ex(landmarks: np.ndarray, rng, augment: bool = True, spatial_affine=None, temporal_mask=None) -> np.ndarray:
    """`spatial_random_affine` on the raw clip, then `apply_augmentations`, then `temporal_mask` (masked frames zeroed) over the augmented
    frames, each only if its option is on.  Returns a new array; the input is not modified."""
    aff, msk = _ranges(spatial_affine, AffineRanges), _ranges(temporal_mask, MaskRanges)
    clip = np.array(landmarks)
    if aff is not None:
        M, shift = _draw_affine(rng, aff)
        clip = affine_xy(clip, M, shift).astype(clip.dtype)
    if augment:
        clip = apply_augmentations(clip, rng)
    if msk is not None:
        m0, m1 = _draw_mask(rng, msk, clip.shape[0])
        clip[m0:m1] = 0
    return clip


def no_augmentation_ex(n_frames: int) -> AugmentationDrawEx:
    return AugmentationDrawEx(no_augmentation(n_frames), _IDENTITY, 0.0, 0, 0)


def fill_clip_table_ex(table: np.ndarray, offsets: np.ndarray, draws: Sequence[AugmentationDrawEx]) -> None:
    """Write one `ishara_clip_aug_ex` row per clip into `table` (a numpy view with the dtype of `_lib.ClipAugEx`)."""
    fill_clip_table(table["base"], offsets, [d.draw for d in draws])
    table["m"] = [d.M for d in draws]
    table["shift_xy"] = [d.shift for d in draws]
    table["m0"] = [d.m0 for d in draws]
    table["m1"] = [d.m1 for d in draws]
    table["reserved"] = 0


class ClipDataset:
    """`ASLDataset.__getitem__` (data_loader.py:166-195) over in-memory raw clips: `(landmarks [n,124,3], phrase)` ->
    `(pad_resize_normalize([apply_augmentations](landmarks), max_frames), phrase)`.  The host path, for `BatchAdapter`.
    `rng` defaults to the `random` module (the reference's global draws).  `spatial_affine` / `temporal_mask` (True: the reference's
    ranges, or an `AffineRanges` / `MaskRanges`) add the two augmentations of `apply_augmentations_ex`, with or without `augment`."""

    def __init__(self, clips, max_frames: int = 384, augment: bool = False, rng=None, spatial_affine=None, temporal_mask=None):
        self.clips, self.max_frames, self.augment = clips, max_frames, augment
        self.rng = random if rng is None else rng
        self.spatial_affine, self.temporal_mask = _ranges(spatial_affine, AffineRanges), _ranges(temporal_mask, MaskRanges)

    def __len__(self) -> int:
        return len(self.clips)

    def __getitem__(self, i):
        lm, phrase = self.clips[i]
        lm = np.asarray(lm, np.float32)
        if self.spatial_affine is not None or self.temporal_mask is not None:
            lm = apply_augmentations_ex(lm, self.rng, self.augment, self.spatial_affine, self.temporal_mask)
        elif self.augment:
            lm = apply_augmentations(lm, self.rng)
        return pad_resize_normalize(lm, self.max_frames), phrase


CLIP_AUG_DTYPE = np.dtype(ClipAug)                 # one ishara_clip_aug row
C_CLIP_AUG_BYTES = CLIP_AUG_DTYPE.itemsize        # 64
CLIP_AUG_EX_DTYPE = np.dtype(ClipAugEx)            # one ishara_clip_aug_ex row
C_CLIP_AUG_EX_BYTES = CLIP_AUG_EX_DTYPE.itemsize  # 96
_LAYOUT_IDS = {"flat": 0, "hands_lips_xy": 1}
_LAYOUT_F = {"flat": 124 * 3, "hands_lips_xy": 224}


def _require_gpu():
    """The device pipeline has no CPU fallback: the library and a GPU are both required."""
    from . import _lib
    import torch
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise _lib.IsharaError("the device input pipeline needs a GPU (there is no CPU fallback)")
    return lib


class DeviceClipStore:
    """The raw clips of a dataset, resident on the device for the whole run: `raw [N_frames,124,3]` f32 with int64 frame
    `offsets` / `lengths` per clip (host copies, for the draws) and the padded phrases `[N,64]` int64 on the device.
    `dataset_or_clips` is an indexable of `(landmarks [n,124,3], phrase)` — the reference's `_load_landmarks(idx)` and
    `_encode_phrase`.  Clips are uploaded in chunks of at most `chunk_bytes` and joined once at the end (the device briefly holds
    the store twice)."""

    def __init__(self, dataset_or_clips, device="cuda:0", chunk_bytes: int = 256 << 20):
        _require_gpu()
        import torch
        self.device = torch.device(device)
        n_clips = len(dataset_or_clips)
        offsets, lengths, phrases = np.zeros(n_clips, np.int64), np.zeros(n_clips, np.int64), []
        chunks, pending, pending_bytes, total = [], [], 0, 0

        def flush():
            nonlocal pending, pending_bytes
            if pending:
                chunks.append(torch.from_numpy(np.concatenate(pending)).to(self.device))
            pending, pending_bytes = [], 0

        for i in range(n_clips):
            lm, phrase = dataset_or_clips[i]
            lm = np.ascontiguousarray(np.asarray(lm.numpy() if hasattr(lm, "numpy") else lm, np.float32))
            if lm.ndim != 3 or lm.shape[1:] != (124, 3):
                raise ValueError(f"clip {i}: landmarks must be [n,124,3], got {lm.shape}")
            offsets[i], lengths[i] = total, lm.shape[0]
            total += lm.shape[0]
            phrases.append(pad_phrase(list(phrase)))
            if lm.shape[0]:
                pending.append(lm)
                pending_bytes += lm.nbytes
            if pending_bytes >= chunk_bytes:
                flush()
        flush()
        if not chunks:                                   # no frames at all: a one-frame store keeps the pointer valid
            chunks = [torch.zeros((1, 124, 3), dtype=torch.float32, device=self.device)]
        self.raw = chunks[0] if len(chunks) == 1 else torch.cat(chunks)
        del chunks
        self.offsets, self.lengths = offsets, lengths
        self.n_frames = total
        self.phrases = torch.from_numpy(np.stack(phrases) if phrases else np.zeros((0, MAX_PHRASE_LENGTH), np.int64)).to(self.device)

    def __len__(self) -> int:
        return len(self.lengths)


class DeviceBatchAdapter:
    """Re-iterable stream of device batches `(x [B,T,F] f32, y [B,64] int64)` built by `ishara_clip_batch` from a
    `DeviceClipStore`: the device twin of `BatchAdapter(ClipDataset(...))`.  It visits the clips in `BatchAdapter`'s order (the
    same `np.random.default_rng(seed)` shuffle) and draws the augmentations per clip in batch order from `rng` (default
    `random.Random(seed)`; pass the `random` module for the reference's global draws).  The per-clip table is written to pinned
    memory, copied asynchronously and consumed by one kernel on the current stream; a pinned table is rewritten only after the
    event of its previous copy has completed.  `shard=(rank, world)`: draw for the whole (global) batch, emit rank's slice.
    `spatial_affine` / `temporal_mask` (True: the reference's ranges, or an `AffineRanges` / `MaskRanges`) add the two augmentations of
    `apply_augmentations_ex`; `emit_lengths=True` yields `(x, y, frame_lengths)` with the clips' frame counts `min(L2, T)` as int32 `[b]`
    on the device, the third element `Model.fit` / `evaluate` accept.  With any of the three on, the batch is built by
    `ishara_clip_batch_ex` from 96-byte rows; with all off, by `ishara_clip_batch` exactly as before (same bits, same draws)."""

    _SLOTS = 3

    def __init__(self, store: DeviceClipStore, batch_size: int, T: int, layout: str = "hands_lips_xy", augment: bool = True,
                 shuffle: bool = False, seed: int = 0, rng=None, drop_last: bool = False, shard: Optional[Tuple[int, int]] = None,
                 spatial_affine=None, temporal_mask=None, emit_lengths: bool = False):
        self._lib = _require_gpu()
        if layout not in _LAYOUT_IDS:
            raise ValueError(f"unknown layout {layout!r}")
        if not 1 <= T <= 4096:
            raise ValueError(f"T={T} unsupported (1..4096)")
        self.store, self.batch_size, self.T, self.layout, self.augment = store, batch_size, T, layout, augment
        self.shuffle, self.drop_last = shuffle, drop_last
        self.spatial_affine, self.temporal_mask = _ranges(spatial_affine, AffineRanges), _ranges(temporal_mask, MaskRanges)
        self.emit_lengths = bool(emit_lengths)
        self._ex = self.spatial_affine is not None or self.temporal_mask is not None or self.emit_lengths
        self._row_bytes = C_CLIP_AUG_EX_BYTES if self._ex else C_CLIP_AUG_BYTES
        self.rank, self.world = shard if shard is not None else (0, 1)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"shard {shard} out of range")
        self.rng = random.Random(seed) if rng is None else rng
        self._order_rng = np.random.default_rng(seed)
        self._slots: List[tuple] = []
        self._turn = 0

    def __len__(self) -> int:
        n = len(self.store)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        order = np.arange(len(self.store))
        if self.shuffle:
            self._order_rng.shuffle(order)
        for i in range(0, len(order), self.batch_size):
            idx = order[i:i + self.batch_size]
            if self.drop_last and len(idx) < self.batch_size:
                break
            yield self.batch(idx)

    def _slot(self):
        """Next pinned table (+ its device copy) of the ring, once the copy of its previous use has completed."""
        import torch
        nbytes = self.batch_size * (self._row_bytes + 8)
        if len(self._slots) < self._SLOTS:
            host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            dev = torch.empty(nbytes, dtype=torch.uint8, device=self.store.device)
            self._slots.append((host, dev, torch.cuda.Event()))
        slot = self._slots[self._turn % len(self._slots)]
        self._turn += 1
        if not slot[2].query():
            slot[2].synchronize()
        return slot

    def batch(self, idx):
        """One device batch of the store's clips `idx` (draws for all of them, emits this rank's slice): `(x, y)`, or
        `(x, y, frame_lengths)` with `emit_lengths`."""
        import torch
        from . import _lib
        idx = np.asarray(idx, np.int64)
        lengths = self.store.lengths[idx]
        if self._ex:
            draws = [draw_augmentation_ex(n, self.rng, self.augment, self.spatial_affine, self.temporal_mask) for n in lengths]
        else:
            draws = [draw_augmentation(n, self.rng) if self.augment else no_augmentation(n) for n in lengths]
        lo, hi = len(idx) * self.rank // self.world, len(idx) * (self.rank + 1) // self.world
        idx, draws = idx[lo:hi], draws[lo:hi]
        b, row = len(idx), self._row_bytes
        host, dev, ev = self._slot()
        hn = host.numpy()
        if self._ex:
            fill_clip_table_ex(hn[:b * row].view(CLIP_AUG_EX_DTYPE), self.store.offsets[idx], draws)
        else:
            fill_clip_table(hn[:b * row].view(CLIP_AUG_DTYPE), self.store.offsets[idx], draws)
        hn[b * row:b * (row + 8)].view(np.int64)[:] = idx
        used = b * (row + 8)
        dev[:used].copy_(host[:used], non_blocking=True)
        ev.record()
        x = torch.empty((b, self.T, _LAYOUT_F[self.layout]), dtype=torch.float32, device=self.store.device)
        y_idx = dev[b * row:used].view(torch.int64)
        if not self._ex:
            _lib.check(self._lib.ishara_clip_batch(_lib.ptr(self.store.raw), _lib.ptr(dev), b, self.T, _LAYOUT_IDS[self.layout],
                                                   _lib.ptr(x), _lib.stream()), "ishara_clip_batch")
            return x, self.store.phrases.index_select(0, y_idx)
        flen = torch.empty(b, dtype=torch.int32, device=self.store.device) if self.emit_lengths else None
        _lib.check(self._lib.ishara_clip_batch_ex(_lib.ptr(self.store.raw), _lib.ptr(dev), b, self.T, _LAYOUT_IDS[self.layout],
                                                  _lib.ptr(x), _lib.ptr(flen), _lib.stream()), "ishara_clip_batch_ex")
        y = self.store.phrases.index_select(0, y_idx)
        return (x, y, flen) if self.emit_lengths else (x, y)
