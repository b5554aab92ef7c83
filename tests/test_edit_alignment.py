"""CPU: the host reference of the edit-operation alignment (evaluation.edit_alignment), ErrorReport's arithmetic and text, and the host side
of ishara_edit_alignment: the exported symbols, the workspace size and the argument refusals of the library and of edit_alignment_device."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import edit_alignment_parity as P
from ishara_amd import _lib, edit_alignment_device
from ishara_amd.evaluation import EditAlignment, ErrorReport, edit_alignment, error_report, levenshtein

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ishara_edit_alignment_workspace_bytes", "ishara_edit_alignment")


def _identities(a, b, al: EditAlignment):
    m, s, d, i = al.ops
    assert s + d + i == levenshtein(list(a), list(b))
    assert m + s + d == len(b) and m + s + i == len(a)
    assert int(al.inserted.sum()) == i and int((al.aligned == -1).sum()) == d
    assert al.aligned.shape == (len(b),) and al.inserted.shape == (len(b) + 1,)


def _replay(pairs):
    """(prediction, target) rebuilt from the script"""
    return [p for _, p in pairs if p != P.PAD], [t for t, _ in pairs if t != P.PAD]


def test_hand_pinned_rows():
    for a, b, ops, aligned, inserted in P.PINNED:
        al = edit_alignment(a, b)
        assert al.ops == ops and al.aligned.tolist() == aligned and al.inserted.tolist() == inserted, (a, b)
        assert edit_alignment(a, b + [P.PAD, 7]).ops == ops                    # the target ends at its first 59


def test_identities_and_replay_on_every_two_symbol_pair():
    seqs = [list(s) for n in range(5) for s in itertools.product((0, 1), repeat=n)]
    assert len(seqs) ** 2 == 961
    for a in seqs:
        for b in seqs:
            al = edit_alignment(a, b)
            _identities(a, b, al)
            assert _replay(al.pairs) == (a, b)


@pytest.mark.parametrize("T,L", P.SHAPES)
@pytest.mark.parametrize("fallback", [False, True])
def test_identities_on_the_case_table(T, L, fallback):
    idx, ln, tg = P.pack(P.cases(T, L), T, L)
    ops, aligned, inserted, conf = P.reference(T, L, fallback)
    P.assert_identities(ops, aligned, inserted, idx, ln, tg, fallback, levenshtein)
    assert conf.sum() == ops.sum() and conf[:59, :59].trace() <= ops[:, 0].sum()
    for c in P.cases(T, L):
        if all(0 <= x < 59 for x in c.pred):
            a = P.prediction(np.asarray(c.pred), min(c.out_len, len(c.pred)), T, False)
            assert _replay(edit_alignment(a, c.target).pairs) == (a, [int(x) for x in c.target]), c.name


def test_the_case_table_covers_what_it_says():
    cs = P.cases(384, 64)
    na = {min(max(c.out_len, 0), 384) for c in cs}
    nb = {len(c.target) for c in cs}
    assert {0, 1, 2, 3, 5, 63, 64, 65, 128, 129, 383, 384} <= na and {0, 1, 2, 63, 64} <= nb
    assert len(cs) % 4 != 0 or len(P.cases(8, 64)) % 4 != 0                   # a partially filled last workgroup somewhere
    assert any(c.out_len < 0 for c in cs) and any(c.out_len > 384 for c in cs)
    assert any(60 in c.pred and 59 in c.pred for c in cs)
    assert {len(c.target) for c in P.cases(384, 40)} >= {0, 1, 2, 40} and max(len(c.target) for c in P.cases(8, 1)) == 1
    ops = P.reference(384, 64, False)[0]
    assert (ops > 0).any(axis=0).all(), "matches, substitutions, deletions and insertions all occur"


def _reports():
    g = np.random.default_rng(5)
    sets = []
    for _ in range(3):
        preds = [g.integers(0, 6, g.integers(0, 9)) for _ in range(7)]
        tgts = [g.integers(0, 6, g.integers(1, 8)) for _ in range(7)]
        sets.append((preds, tgts))
    return sets


def test_error_report_arithmetic():
    sets = _reports()
    a, b, c = (error_report(p, t, max_len=8) for p, t in sets)
    assert (a + b) + c == a + (b + c)
    whole = error_report(sum((p for p, _ in sets), []), sum((t for _, t in sets), []), max_len=8)
    assert a + b + c == whole and whole.n_clips == 21
    assert a + ErrorReport() == a and not (a == b)
    m = whole.confusion
    assert m.dtype == np.int64 and m.shape == (60, 60) and m[59, 59] == 0
    assert whole.matches == m[:59, :59].trace()
    assert whole.substitutions == m[:59, :59].sum() - m[:59, :59].trace()
    assert whole.deletions == m[:59, 59].sum() and whole.insertions == m[59, :59].sum()
    assert whole.position_counts.tolist() == [sum(len(t) > j for _, ts in sets for t in ts) for j in range(8)]
    assert whole.position_errors.sum() == whole.substitutions + whole.deletions
    assert whole.insert_positions.shape == (9,) and whole.insert_positions.sum() == whole.insertions
    pc = whole.per_char()
    assert sum(v["occurrences"] for v in pc["target"].values()) == m[:59].sum()
    assert sum(v["correct"] for v in pc["target"].values()) == whole.matches
    assert sum(v["substituted"] for v in pc["target"].values()) == whole.substitutions
    assert sum(v["deleted"] for v in pc["target"].values()) == whole.deletions
    assert sum(pc["inserted"].values()) == whole.insertions
    # the arrays of the device entry give the same report as the alignments
    idx = np.full((21, 8), -1, np.int32)
    tg = np.full((21, 8), 59, np.int32)
    ln = np.zeros(21, np.int32)
    for k, (p, t) in enumerate(zip(sum((p for p, _ in sets), []), sum((t for _, t in sets), []))):
        idx[k, :len(p)], ln[k], tg[k, :len(t)] = p, len(p), t
    assert ErrorReport.from_arrays(*P.reference_of(idx, ln, tg, False), tg) == whole


def test_error_report_fallback_replaces_short_predictions():
    from ishara_amd.tflite_model import FALLBACK_PHRASE
    t = [[1, 2, 3]] * 3
    with_fb = error_report([[1, 2], [], [1, 2, 3]], t, fallback=True)
    assert with_fb == error_report([list(FALLBACK_PHRASE), list(FALLBACK_PHRASE), [1, 2, 3]], t)
    assert not (with_fb == error_report([[1, 2], [], [1, 2, 3]], t))


def test_most_confused_order():
    m = np.zeros((60, 60), np.int64)
    m[3, 3], m[4, 2], m[2, 4], m[7, 1], m[1, 59], m[59, 1], m[5, 6] = 50, 3, 3, 9, 40, 40, 3
    r = ErrorReport(confusion=m)
    assert r.most_confused(10) == [(7, 1, 9), (2, 4, 3), (4, 2, 3), (5, 6, 3)]      # count, then (target, predicted); no diagonal, no "nothing"
    assert r.most_confused(2) == [(7, 1, 9), (2, 4, 3)]


def test_format_is_a_fixed_table():
    r = error_report([[1, 2, 3], [5, 6], [1, 1]], [[3, 1, 2], [6, 5], [1, 59, 59]])
    text = r.format({i: chr(97 + i) for i in range(26)}, k=3)
    assert text == ("clips 3  matches 3  substitutions 2  deletions 1  insertions 2\n"
                    "  # tgt pred  count\n"
                    "  0   f    g      1\n"
                    "  1   g    f      1\n"
                    "deleted : d:1\n"
                    "inserted: b:1 d:1")
    assert ErrorReport().format({}) == ("clips 0  matches 0  substitutions 0  deletions 0  insertions 0\n"
                                        "  # tgt pred  count\n"
                                        "deleted : -\n"
                                        "inserted: -")


def test_new_symbols_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_workspace_bytes_monotone_and_non_negative(lib):
    f = lib.ishara_edit_alignment_workspace_bytes
    assert f(0, 384) == 0
    for T in (1, 8, 11, 12, 384, 4096):
        sizes = [f(B, T) for B in (0, 1, 5, 256, 4096)]
        assert all(s >= 0 for s in sizes) and sizes == sorted(sizes)
        assert all(f(B, T) >= B * T * 16 for B in (1, 256))                      # two 8-byte ballots per table row
    for B in (1, 7, 256):
        sizes = [f(B, T) for T in (1, 8, 11, 12, 383, 384, 4096)]
        assert sizes == sorted(sizes)
        assert f(B, 1) >= B * 11 * 16                                            # the fallback phrase has more rows than a short T
    assert f(-1, 384) < 0 and f(4, 0) < 0 and f(4, 4097) < 0                     # outside the entry's limits: no size


def test_entry_point_rejects_bad_arguments(lib):
    """Argument checks run on the host before any launch: no device needed."""
    f, null = lib.ishara_edit_alignment, None
    assert f(null, null, 4, 384, null, 65, 1, null, null, null, null, null, null) != 0
    assert b"L=65" in lib.ishara_last_error()
    assert f(null, null, 4, 384, null, 0, 1, null, null, null, null, null, null) != 0
    assert f(null, null, 4, 0, null, 64, 1, null, null, null, null, null, null) != 0
    assert b"T=0" in lib.ishara_last_error()
    assert f(null, null, 4, 4097, null, 64, 1, null, null, null, null, null, null) != 0
    assert f(null, null, -1, 384, null, 64, 1, null, null, null, null, null, null) != 0
    assert b"B=-1" in lib.ishara_last_error()
    assert f(null, null, 4, 384, null, 64, 1, null, null, null, null, null, null) != 0      # null buffers
    assert b"null" in lib.ishara_last_error()
    assert f(256, 256, 4, 384, 256, 64, 1, 256, 256, 256, null, null, null) != 0            # null workspace (the matrix may be null)
    assert b"null workspace" in lib.ishara_last_error()
    assert f(256, 256, 4, 384, 256, 64, 1, 256, 256, 256, 256, 264, null) != 0
    assert b"16-byte" in lib.ishara_last_error()
    assert f(null, null, 0, 384, null, 64, 0, null, null, null, null, null, null) == 0      # B = 0: a no-op


def test_device_entry_refuses_before_touching_the_library():
    idx, ln, tg = torch.zeros((2, 8), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.full((2, 4), 59, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        edit_alignment_device(idx, ln, tg)
    with pytest.raises(ValueError, match="torch tensor"):
        edit_alignment_device(idx.numpy(), ln, tg)
