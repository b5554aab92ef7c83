"""GPU: the edit-operation alignment (csrc/score_align.hip, ishara_edit_alignment) equals the host reference exactly -- ops, aligned,
inserted and the confusion matrix, array_equal on the case table of edit_alignment_parity.py -- writes nothing outside its outputs and its
workspace, accumulates its matrix, and agrees with ishara_edit_distance; BatchedTFLiteModel.score(breakdown=True) and
CallbackEval(error_report=True) give the host's report of their own decodes and leave what they returned before unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import edit_alignment_parity as P
from ishara_amd import _lib, edit_alignment_device, get_model
from ishara_amd.evaluation import CallbackEval, ErrorReport, error_report, levenshtein, make_num_to_char
from ishara_amd.tflite_batch import BatchedTFLiteModel, apply_fallback, encode_phrase

pytestmark = pytest.mark.gpu

SENTINEL = -77
GUARD = 64                 # int32 guard words behind every output and behind the workspace
SMALL = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(lib, idx, ln, tg, fallback, want_conf=True, conf=None):
    """One launch on sentinel-filled outputs with guard words behind each and behind the workspace -> (ops, aligned, inserted, confusion)
    as host int32 arrays; asserts that every guard word survived."""
    B, T = idx.shape
    L = tg.shape[1]
    d_idx, d_ln, d_tg = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (idx, ln, tg))
    sizes = (B * 4, B * L, B * (L + 1))
    outs = [torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for n in sizes]
    need = int(lib.ishara_edit_alignment_workspace_bytes(B, T))
    assert need >= 0
    ws = torch.full((need + 256 + GUARD * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    ws_at = (-ws.data_ptr()) % 256
    if want_conf and conf is None:
        conf = torch.zeros((60, 60), dtype=torch.int32, device="cuda")
    _lib.check(lib.ishara_edit_alignment(_lib.ptr(d_idx), _lib.ptr(d_ln), B, T, _lib.ptr(d_tg), L, int(fallback), _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                         _lib.ptr(outs[2]), _lib.ptr(conf) if want_conf else None, C.c_void_p(ws.data_ptr() + ws_at), _stream()),
               "ishara_edit_alignment")
    host = [o.cpu().numpy() for o in outs]
    for name, h, n in zip(P.NAMES, host, sizes):
        assert (h[n:] == SENTINEL).all(), f"{name}: words behind the output were written"
    w = ws.cpu().numpy()
    assert (w[:ws_at] == 0xA5).all() and (w[ws_at + need:] == 0xA5).all(), "bytes outside the workspace were written"
    return (host[0][:sizes[0]].reshape(B, 4), host[1][:sizes[1]].reshape(B, L), host[2][:sizes[2]].reshape(B, L + 1),
            conf.cpu().numpy() if want_conf else None)


@pytest.mark.parametrize("T,L", P.SHAPES)
@pytest.mark.parametrize("fallback", [False, True])
def test_case_table_equals_the_host_reference(lib, T, L, fallback):
    idx, ln, tg = P.pack(P.cases(T, L), T, L)
    got = _launch(lib, idx, ln, tg, fallback)
    want = P.reference(T, L, fallback)
    assert (got[0] != SENTINEL).all() and (got[1] != SENTINEL).all() and (got[2] != SENTINEL).all(), "an output entry was not written"
    assert not P.mismatches(got, want), P.mismatches(got, want)
    P.assert_identities(got[0], got[1], got[2], idx, ln, tg, fallback, levenshtein)
    if fallback:                                                   # the distance kernel on the same buffers
        B = idx.shape[0]
        d_idx, d_ln, d_tg = (torch.from_numpy(a).cuda() for a in (idx, ln, tg))
        dist, tlen = (torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2))
        _lib.check(lib.ishara_edit_distance(_lib.ptr(d_idx), _lib.ptr(d_ln), B, T, _lib.ptr(d_tg), L, _lib.ptr(dist), _lib.ptr(tlen), _stream()),
                   "ishara_edit_distance")
        assert np.array_equal(got[0][:, 1:].sum(axis=1), dist.cpu().numpy())
        assert np.array_equal(got[0][:, :3].sum(axis=1), tlen.cpu().numpy())
    # B = 1 and B = 5: a single wave, and a second workgroup with one wave at work
    for B in (1, 5):
        part = _launch(lib, idx[:B], ln[:B], tg[:B], fallback)
        assert not P.mismatches(part, P.reference_of(idx[:B], ln[:B], tg[:B], fallback))


def test_matrix_accumulates_null_matrix_and_determinism(lib):
    T, L = 384, 64
    idx, ln, tg = P.pack(P.cases(T, L), T, L)
    first = _launch(lib, idx, ln, tg, True)
    conf = torch.from_numpy(first[3].copy()).cuda()
    again = _launch(lib, idx, ln, tg, True, conf=conf)
    assert np.array_equal(again[3], 2 * first[3]), "a second launch into the same matrix does not give twice the first"
    assert not P.mismatches(again[:3], first[:3]), "a second identical launch gives other integers"
    none = _launch(lib, idx, ln, tg, True, want_conf=False)
    assert not P.mismatches(none[:3], first[:3]), "confusion = NULL changes the per-clip outputs"


def test_refusals(lib):
    B, T = 4, 8
    idx, ln = torch.zeros((B, T), dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    wide = torch.full((B, 65), 59, dtype=torch.int32, device="cuda")
    out = torch.zeros(B * 66, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rc = lib.ishara_edit_alignment(_lib.ptr(idx), _lib.ptr(ln), B, T, _lib.ptr(wide), 65, 0, _lib.ptr(out), _lib.ptr(out), _lib.ptr(out), None,
                                   _lib.ptr(ws), _stream())
    assert rc != 0 and b"L=65" in lib.ishara_last_error()
    with pytest.raises(ValueError, match="L=65"):
        edit_alignment_device(idx, ln, wide)
    tg = wide[:, :8].contiguous()
    with pytest.raises(ValueError, match="int32"):
        edit_alignment_device(idx.long(), ln, tg)
    with pytest.raises(ValueError, match="dimension"):
        edit_alignment_device(idx[0], ln, tg)
    with pytest.raises(ValueError, match="disagree"):
        edit_alignment_device(idx, ln[:2], tg)
    with pytest.raises(ValueError, match="GPU"):
        edit_alignment_device(idx, ln.cpu(), tg)
    with pytest.raises(ValueError, match="too small"):
        edit_alignment_device(idx, ln, tg, workspace=torch.zeros(64, dtype=torch.uint8, device="cuda"))


def test_device_entry_equals_the_host_reference_and_accumulates():
    T, L = 8, 40
    idx, ln, tg = P.pack(P.cases(T, L), T, L)
    d = [torch.from_numpy(a).cuda() for a in (idx, ln, tg)]
    for fallback in (False, True):
        ops, aligned, inserted, conf = edit_alignment_device(*d, fallback=fallback)
        assert not P.mismatches([t.cpu().numpy() for t in (ops, aligned, inserted, conf)], P.reference(T, L, fallback))
    ws = torch.zeros(int(_lib.load().ishara_edit_alignment_workspace_bytes(idx.shape[0], T)) + 16, dtype=torch.uint8, device="cuda")
    _, _, _, conf2 = edit_alignment_device(*d, fallback=True, confusion=conf, workspace=ws)
    assert conf2 is conf and np.array_equal(conf.cpu().numpy(), 2 * P.reference(T, L, True)[3])


# ------------------------------------------------------------------------------------------------ the small model end to end
def _clip(n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, 276)).astype(np.float32)
    x[g.random((n, 276)) < 0.05] = np.nan
    return x


@pytest.mark.parametrize("beam_width", [0, 4])
def test_score_breakdown_equals_the_host_report(monkeypatch, beam_width):
    monkeypatch.setenv("ISHARA_WS_GUARD", "1")
    model = get_model(**SMALL, dtype="f32", max_batch=8, seed=5)
    g = np.random.default_rng(31 + beam_width)
    lengths = [0, 1, 176, 300, 40, 7, 400, 90, 250, 12, 333, 64]      # 12 clips, batch size 5: two whole batches and a partial one
    clips = [_clip(n, 4000 + i) for i, n in enumerate(lengths)]
    targets = [g.integers(0, 59, int(k)) for k in g.integers(1, 65, len(clips))]
    kw = dict(batch_size=5, max_frames=512, beam_width=beam_width)
    graph = BatchedTFLiteModel(model, use_graph=True, **kw)
    eager = BatchedTFLiteModel(model, use_graph=False, **kw)
    plain = graph.score(clips, targets)
    res = graph.score(clips, targets, breakdown=True)
    res_e = eager.score(clips, targets, breakdown=True)
    L = graph.L
    enc = np.stack([encode_phrase(t, None, L) for t in targets])
    preds = graph.predict_indices(clips)
    T = graph.T
    idx, ln = np.full((len(preds), T), -1, np.int32), np.zeros(len(preds), np.int32)
    for b, p in enumerate(preds):
        idx[b, :len(p)], ln[b] = p, len(p)
    want = P.reference_of(idx, ln, enc, True)
    for r, what in ((res, "graph"), (res_e, "eager")):
        assert not P.mismatches((r["ops"], r["aligned"], r["inserted"], r["report"].confusion), want), what
        assert r["report"] == error_report([apply_fallback(p) for p in preds], enc, max_len=L), what
        assert r["report"].n_clips == len(clips)
        assert r["mean_score"] == plain["mean_score"] and np.array_equal(r["scores"], plain["scores"]), what
        assert np.array_equal(r["distances"], plain["distances"]), what
        assert np.array_equal(r["ops"][:, 1:].sum(axis=1), plain["distances"]), what
    assert set(plain) == {"mean_score", "scores", "distances"}
    again = graph.score(clips, targets, breakdown=True)                # the matrix is zeroed per call
    assert again["report"] == res["report"]
    _lib.check(model._lib.ishara_workspace_guard_check(model._h), "workspace guard")


def test_callback_eval_error_report():
    from oracle import ishara_oracle as O
    kw = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(48, 36))
    model = get_model(**kw, dtype="f32", max_batch=4, device="cuda:0", seed=0)
    ocfg = O.Config(**kw)
    data = [O.synthetic_batch(ocfg, 4, seed=1), O.synthetic_batch(ocfg, 3, seed=2)]
    num_to_char = make_num_to_char({chr(ord("a") + i % 26) + str(i // 26): i for i in range(59)})
    base_lines, lines, logs0, logs = [], [], {}, {}
    base = CallbackEval(data, num_to_char, n_show=2, weights_path=None, printer=base_lines.append)
    base.set_model(model)
    base.on_epoch_end(0, logs0)
    cb = CallbackEval(data, num_to_char, n_show=2, weights_path=None, printer=lines.append, error_report=True, n_confusions=5)
    cb.set_model(model)
    cb.on_epoch_end(0, logs)
    preds, tgts = [], []
    for x, y in data:
        preds += model.decode_batch(model(x, training=False))
        tgts += list(y)
    want = error_report(preds, tgts, max_len=64)
    assert isinstance(cb.last_report, ErrorReport) and cb.last_report == want
    assert cb.last_score == base.last_score and base.last_report is None
    assert lines[:len(base_lines)] == base_lines and "\n".join(lines[len(base_lines):]) == want.format(num_to_char, 5)
    assert logs0 == {"val_levenshtein": base.last_score}
    assert logs == {"val_levenshtein": base.last_score, "val_substitutions": want.substitutions, "val_deletions": want.deletions,
                    "val_insertions": want.insertions}
