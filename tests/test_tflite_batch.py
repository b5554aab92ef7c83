"""CPU: the host side of BatchedTFLiteModel (ishara_amd/tflite_batch.py) — packing, offsets and partial-batch padding, phrase
encoding, the len < 3 fallback, the constructor's checks — and the two new C-ABI entry points in the header, the library and SIGNATURES."""
import os
import re

import numpy as np
import pytest

from ishara_amd import _lib, make_config
from ishara_amd import tflite_batch as TB
from ishara_amd.evaluation import mean_score
from ishara_amd.model import Model
from ishara_amd.tflite_model import FALLBACK_PHRASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ishara_preprocess_batch", "ishara_edit_distance")


def _clips(lengths, seed=0):
    g = np.random.default_rng(seed)
    return [g.standard_normal((n, 276)).astype(np.float32) for n in lengths]


def test_batch_offsets_pad_with_empty_clips():
    off = TB.batch_offsets([3, 0, 5], 6)
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 3, 8, 8, 8, 8]
    assert TB.batch_offsets([], 2).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        TB.batch_offsets([1, 2, 3], 2)


def test_pack_clips_back_to_back():
    clips = _clips([4, 0, 7, 1])
    raw = np.full((20, 276), np.inf, np.float32)
    off = np.empty(6, np.int64)
    rows = TB.pack_clips(clips, raw, off)
    assert rows == 12 and off.tolist() == [0, 4, 4, 11, 12, 12]
    for c, a, b in zip(clips, off[:-1], off[1:]):
        assert np.array_equal(raw[a:b], c)
    assert np.isinf(raw[12:]).all()                 # nothing past the used rows is touched
    with pytest.raises(ValueError, match="capacity"):
        TB.pack_clips(_clips([15, 10]), raw, np.empty(3, np.int64))


def test_check_clip_and_packed_input():
    with pytest.raises(ValueError):
        TB.check_clip(np.zeros((5, 275)), 10)
    with pytest.raises(ValueError, match="max_frames"):
        TB.check_clip(np.zeros((11, 276)), 10)
    assert TB.check_clip(np.zeros((0, 276), np.float64), 10).dtype == np.float32
    frames = np.zeros((9, 276), np.float32)
    f, o = TB.check_packed(frames, np.array([0, 4, 4, 9], np.int32), 8)
    assert o.dtype == np.int64 and o.tolist() == [0, 4, 4, 9]
    for bad in ([0, 5, 3], [0, 10], [-1, 3], [0, 9.0]):
        with pytest.raises(ValueError):
            TB.check_packed(frames, np.array(bad), 8)
    with pytest.raises(ValueError, match="max_frames"):
        TB.check_packed(frames, np.array([0, 9]), 8)


def test_encode_phrase():
    c2n = {"a": 0, "b": 1, " ": 2, "z": 58}
    enc = TB.encode_phrase("ab z", c2n, 8)
    assert enc.dtype == np.int32 and enc.tolist() == [0, 1, 2, 58, 59, 59, 59, 59]
    assert TB.encode_phrase([3, 4], None, 3).tolist() == [3, 4, 59]
    assert TB.encode_phrase(np.arange(58, -6, -1) % 59, None, 64).shape == (64,)     # a full-length target has no pad
    with pytest.raises(ValueError, match="not in char_to_num"):
        TB.encode_phrase("abc", c2n, 8)                 # unknown character
    with pytest.raises(ValueError, match="empty"):
        TB.encode_phrase("", c2n, 8)                    # c18 would divide by zero
    with pytest.raises(ValueError, match="empty"):
        TB.encode_phrase([], None, 8)
    with pytest.raises(ValueError, match="max_label_len"):
        TB.encode_phrase("a" * 9, c2n, 8)
    with pytest.raises(ValueError, match="char_to_num"):
        TB.encode_phrase("ab", None, 8)
    for bad in ([59], [-1], [1, 60]):                  # the pad index is not a symbol
        with pytest.raises(ValueError):
            TB.encode_phrase(bad, None, 8)


def test_fallback_rule_and_one_hot():
    for n in (0, 1, 2):
        assert TB.apply_fallback(np.arange(n)) is FALLBACK_PHRASE
    x = np.array([5, 6, 7])
    assert TB.apply_fallback(x) is x
    oh = TB.one_hot(np.array([0, 58, 59]))
    assert oh.shape == (3, 59) and oh[0, 0] == 1 and oh[1, 58] == 1 and not oh[2].any()


def test_fallback_constant_in_kernel_equals_wrapper():
    csrc = os.path.join(ROOT, "ishara_amd", "csrc")
    src = open(os.path.join(csrc, "edit_distance.h")).read()
    m = re.search(r"__constant__ int fallback_phrase\[FALLBACK_LEN\] = \{([^}]*)\}", src)
    assert m, "edit_distance.h: fallback_phrase not found"
    assert [int(v) for v in m.group(1).split(",")] == FALLBACK_PHRASE.tolist()
    assert int(re.search(r"constexpr int FALLBACK_LEN = (\d+);", src).group(1)) == len(FALLBACK_PHRASE)
    # every kernel takes the phrase from that header: no .hip file keeps an array of its own
    hips = [f for f in sorted(os.listdir(csrc)) if f.endswith(".hip")]
    assert hips
    for f in hips:
        assert not re.search(r"\{\s*17\s*,\s*0\s*,\s*32\s*,", open(os.path.join(csrc, f)).read()), f"{f}: a fallback phrase of its own"


def test_normalized_scores_equal_host_mean_score():
    g = np.random.default_rng(1)
    alphabet = "abcdefghij"
    preds = ["".join(g.choice(list(alphabet), g.integers(0, 12))) for _ in range(50)]
    tgts = ["".join(g.choice(list(alphabet), g.integers(1, 12))) for _ in range(50)]
    from ishara_amd.evaluation import levenshtein
    dist = np.array([levenshtein(p, t) for p, t in zip(preds, tgts)], np.int32)
    tlen = np.array([len(t) for t in tgts], np.int32)
    mean, scores = TB.normalized_scores(dist, tlen)
    assert mean == mean_score(preds, tgts) and scores.dtype == np.float64


def test_constructor_checks_without_a_device():
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276), max_batch=4), device=None)
    with pytest.raises(ValueError, match="batch_size"):
        TB.BatchedTFLiteModel(m, batch_size=8)
    with pytest.raises(ValueError, match="batch_size"):
        TB.BatchedTFLiteModel(m, batch_size=0)
    with pytest.raises(ValueError, match="max_frames"):
        TB.BatchedTFLiteModel(m, batch_size=4, max_frames=9000)
    with pytest.raises(ValueError, match="no device"):
        TB.BatchedTFLiteModel(m, batch_size=4)
    wrong_f = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 224), max_batch=4), device=None)
    with pytest.raises(ValueError, match="276"):
        TB.BatchedTFLiteModel(wrong_f, batch_size=4)
    long_labels = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276), max_batch=4,
                                    max_label_len=65), device=None)
    with pytest.raises(ValueError, match="max_label_len"):
        TB.BatchedTFLiteModel(long_labels, batch_size=4)


def test_new_symbols_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_entry_points_reject_bad_arguments(lib):
    """Argument checks run on the host before any launch: no device needed."""
    null = None
    assert lib.ishara_edit_distance(null, null, 4, 384, null, 65, null, null, null) != 0
    assert b"L=65" in lib.ishara_last_error()
    assert lib.ishara_edit_distance(null, null, 4, 384, null, 0, null, null, null) != 0
    assert lib.ishara_edit_distance(null, null, 4, 384, null, 64, null, null, null) != 0      # null buffers
    assert lib.ishara_preprocess_batch(null, 0, null, 4, 9000, null, null, null, 384, null) != 0
    assert b"max_frames" in lib.ishara_last_error()
    assert lib.ishara_preprocess_batch(null, 0, null, 4, 1024, null, null, null, 0, null) != 0
    assert lib.ishara_preprocess_batch(16, 10, 256, 4, 1024, 256, 256, 260, 384, null) != 0
    assert b"16-byte" in lib.ishara_last_error()
