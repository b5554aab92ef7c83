"""GPU: ishara_logits_combine (csrc/logits_combine.hip) against the fp64 reference over the case table of tests/ensemble_parity.py, its
contract (every element written, nothing read that must not be, 4-byte alignment, determinism, graph replay with rewritten weights), the
chain combine_logits -> ctc_greedy_decode -> ishara_edit_distance on a synthetic ensemble, and EnsembleTFLiteModel on three small models."""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_parity as P
from decode_check import check_decode_parity, frame_margins
from ishara_amd import _lib, get_model
from ishara_amd.ctc import ctc_beam_decode, ctc_greedy_decode, greedy_decode_device
from ishara_amd.ctc_beam import CharBigramLM
from ishara_amd.ensemble import EnsembleTFLiteModel, combine_logits, combine_reference
from ishara_amd.evaluation import levenshtein, mean_score
from ishara_amd.tflite_batch import BatchedTFLiteModel, apply_fallback, encode_phrase
from oracle import ishara_oracle as O

pytestmark = pytest.mark.gpu

CHARS = " !#$%&'()*+,-./0123456789:;=?@[_abcdefghijklmnopqrstuvwxyz~"
CHAR_TO_NUM = {c: i for i, c in enumerate(CHARS)}
Cn, BLANK = 60, 59
SMALL = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276))
CASES = {c["name"]: c for c in P.cases()}


def _dev(a, offset=0):
    """a numpy array on the device, `offset` elements into its allocation (offset 1: an address that is 4-byte aligned and no more)"""
    a = np.array(a)                                      # a writable copy: the cases' arrays are read-only
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = buf[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert offset == 0 or view.data_ptr() % 8 == 4
    return view


def _launch(lib, xs, w, it, fl, mode, out):
    M = len(xs)
    B, T, Cc = xs[0].shape
    arr = (C.c_void_p * M)(*[x.data_ptr() for x in xs])
    _lib.check(lib.ishara_logits_combine(None, arr, M, B, T, Cc, _lib.ptr(w), _lib.ptr(it), mode, _lib.ptr(fl), _lib.ptr(out), _lib.stream()),
               "ishara_logits_combine")


def _device_case(case, offset=0):
    xs = [_dev(x, offset) for x in case["logits"]]
    w = _dev(case["weights"], offset)
    it = None if case["inv_temp"] is None else _dev(case["inv_temp"], offset)
    fl = None if case["frame_len"] is None else _dev(case["frame_len"], offset)
    out = _dev(np.full((case["B"], case["T"], case["C"]), np.nan, np.float32), offset)       # poisoned: every element must be written
    return xs, w, it, fl, out


def _run(lib, case, offset=0):
    xs, w, it, fl, out = _device_case(case, offset)
    _launch(lib, xs, w, it, fl, case["mode"], out)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the operator
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_within_the_bound(lib, name):
    """every element of a NaN-poisoned `out` is written; the rows inside their clips are within K * 2^-24 * scale of the fp64 reference;
    rows past a clip's end are +0 although the inputs hold NaN there; a model under a zero weight holds NaN and is not read"""
    case = CASES[name]
    ratio = P.compare(case, _run(lib, case))
    print(f"{name}: err / bound {ratio:.4f} (K = {P.K})")
    assert ratio <= 1.0, f"{name}: err / bound {ratio}"


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n]["B"] * CASES[n]["T"] == 134 and CASES[n]["C"] in (59, 60, 63)])
def test_buffers_aligned_to_four_bytes_only(lib, name):
    case = CASES[name]
    got = _run(lib, case, offset=1)
    assert P.compare(case, got) <= 1.0
    assert np.array_equal(got.view(np.uint32), _run(lib, case).view(np.uint32)), "the result depends on the buffers' alignment"


def test_two_runs_are_bit_identical(lib):
    for name in sorted(CASES)[::7]:
        a, b = _run(lib, CASES[name]), _run(lib, CASES[name])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


@pytest.mark.parametrize("mode", [0, 1])
def test_graph_replay_reads_rewritten_weights_and_temperatures(lib, mode):
    g = np.random.default_rng(31 + mode)
    M, B, T = 3, 3, 37
    xs = [_dev((2 * g.standard_normal((B, T, Cn))).astype(np.float32)) for _ in range(M)]
    w, it = _dev(np.array([0.2, 0.5, 0.3], np.float32)), _dev(np.array([1.0, 0.5, 2.0], np.float32))
    out = torch.full((B, T, Cn), float("nan"), device="cuda")
    _launch(lib, xs, w, it, None, mode, out)                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(lib, xs, w, it, None, mode, out)
    first = out.clone()
    w.copy_(torch.tensor([0.6, 0.0, 0.4], device="cuda"))        # one model drops out: the branch is per launch, not per capture
    it.copy_(torch.tensor([0.7, 1.0, 1.5], device="cuda"))
    out.fill_(float("nan"))
    graph.replay()
    replayed = out.clone()
    eager = torch.full_like(out, float("nan"))
    _launch(lib, xs, w, it, None, mode, eager)
    torch.cuda.synchronize()
    assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32))
    assert not torch.equal(replayed, first)
    ref = combine_reference([x.cpu().numpy() for x in xs], [0.6, 0.0, 0.4], "linear" if mode else "log_linear", 1.0 / np.array([0.7, 1.0, 1.5], np.float32).astype(np.float64))
    assert np.abs(replayed.cpu().numpy() - ref).max() < 1e-4


def test_combine_logits_matches_the_abi_and_lends_the_profiler(lib):
    g = np.random.default_rng(8)
    xs = [(2 * g.standard_normal((5, 33, Cn))).astype(np.float32) for _ in range(3)]
    fl = [33, 1, 20, 33, 7]
    got = combine_logits([torch.from_numpy(x).cuda() for x in xs], [1, 2, 1], "linear", [1.0, 0.5, 2.0], fl).cpu().numpy()
    ref = combine_reference(xs, [0.25, 0.5, 0.25], "linear", [1.0, 0.5, 2.0], fl)
    assert np.abs(got - ref).max() < 1e-4 and (got[1, 1:] == 0).all()
    stacked = combine_logits(torch.from_numpy(np.stack(xs)).cuda(), [1, 2, 1], "linear", [1.0, 0.5, 2.0], torch.tensor(fl, device="cuda"))
    assert np.array_equal(stacked.cpu().numpy().view(np.uint32), got.view(np.uint32))
    with pytest.raises(ValueError):
        combine_logits([torch.from_numpy(xs[0]).cuda()] * 9)
    with pytest.raises(_lib.IsharaError):
        combine_logits([torch.from_numpy(xs[0])])
    # a handle lends its profiler: one record under the key logits_combine with (M + 1) * B * T * C * 4 bytes
    model = get_model(**SMALL, dtype="f32", max_batch=2, seed=1)
    d = [_dev(x) for x in xs]
    out = torch.empty((5, 33, Cn), device="cuda")
    arr = (C.c_void_p * 3)(*[x.data_ptr() for x in d])
    _lib.check(lib.ishara_profile_enable(model._h, 1))
    try:
        _lib.check(lib.ishara_logits_combine(model._h, arr, 3, 5, 33, Cn, _lib.ptr(_dev(np.ones(3, np.float32))), None, 0, None, _lib.ptr(out), _lib.stream()))
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 16)
        assert lib.ishara_profile_report(model._h, buf, len(buf)) >= 0
    finally:
        lib.ishara_profile_enable(model._h, 0)
    rows = {ln.split()[0]: ln.split()[1:] for ln in buf.value.decode().splitlines()}
    assert "logits_combine" in rows and int(rows["logits_combine"][0]) == 1 and float(rows["logits_combine"][2]) == 4 * 5 * 33 * Cn * 4


# ------------------------------------------------------------------------------------------------ 2. the chain on a synthetic ensemble
def _synthetic(seed=0, B=16, T=64, M=4, sharp=4.0, noise=1.6):
    """confident alignments (runs of 2..4 frames of a character or the blank, 8 blank frames at the end) as logits of height `sharp`, and M
    "models": the truth plus independent N(0, noise^2) on every logit.  Returns (models float32 [M, B, T, C], the phrases)."""
    g = np.random.default_rng(seed)
    x, phrases = np.zeros((B, T, Cn)), []
    for b in range(B):
        t, lab, prev = 0, [], None
        while t < T - 8:
            n = int(g.integers(2, 5))
            c = BLANK if (prev is not None and prev != BLANK and g.random() < 0.5) else int(g.integers(0, BLANK))
            if c == prev:
                c = BLANK
            x[b, t:min(t + n, T - 8), c] += sharp
            if c != BLANK:
                lab.append(c)
            prev, t = c, t + n
        x[b, T - 8:, BLANK] += sharp
        phrases.append(lab)
    return np.stack([x + noise * g.standard_normal(x.shape) for _ in range(M)]).astype(np.float32), phrases


def _host_scores(decodes, phrases):
    """(mean of (len(target) - Levenshtein) / len(target), the distances) with the wrapper's len < 3 fallback, as ishara_edit_distance has it"""
    d = [levenshtein([int(v) for v in apply_fallback(np.asarray(p, np.int64))], t) for p, t in zip(decodes, phrases)]
    return float(np.mean([(len(t) - k) / len(t) for k, t in zip(d, phrases)])), d


def _device_distances(lib, x_dev, phrases):
    idx, ln = greedy_decode_device(x_dev)
    B, T = idx.shape
    tg = torch.from_numpy(np.stack([encode_phrase(np.asarray(p), None, 64) for p in phrases])).cuda()
    dist, tlen = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(lib.ishara_edit_distance(_lib.ptr(idx), _lib.ptr(ln), B, T, _lib.ptr(tg), 64, _lib.ptr(dist), _lib.ptr(tlen), _lib.stream()), "ishara_edit_distance")
    return dist.cpu().numpy().tolist(), tlen.cpu().numpy().tolist()


@pytest.mark.parametrize("mode", ["log_linear", "linear"])
def test_synthetic_ensemble_beats_its_best_member(lib, mode):
    models, phrases = _synthetic()
    xs = [torch.from_numpy(m).cuda() for m in models]
    fused = combine_logits(xs, mode=mode)
    ref = combine_reference(list(models), None, mode)
    got = fused.cpu().numpy()
    decodes = ctc_greedy_decode(fused)
    rec = check_decode_parity(ref, got, decodes, O.decode_phrase, require_clips=1, what=f"fused {mode} vs fp64")
    dist, tlen = _device_distances(lib, fused, phrases)
    score, host_dist = _host_scores(decodes, phrases)
    assert dist == host_dist and tlen == [len(p) for p in phrases]
    singles = [_host_scores(ctc_greedy_decode(x), phrases)[0] for x in xs]
    print(f"{mode}: ensemble {score:.3f}, single models {[round(s, 3) for s in singles]}, {rec['clips_compared']} clips fully resolved")
    assert score >= max(singles) + 0.5, (score, singles)


# ------------------------------------------------------------------------------------------------ 3. the wrapper
def _clip(n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, 276)).astype(np.float32)
    x[g.random(n) < 0.3, :42] = np.nan
    return x


@pytest.fixture(scope="module")
def trio():
    """three small models from different seeds, one of them in another compute dtype; ten ragged clips, one of them empty (batch_size 4:
    the last batch is partial); targets; the logits the ensemble computed, read once"""
    models = [get_model(**SMALL, dtype="f32", max_batch=4, seed=5), get_model(**SMALL, dtype="bf16", max_batch=4, seed=6),
              get_model(**SMALL, dtype="f32", max_batch=8, seed=7)]
    g = np.random.default_rng(12)
    lengths = [int(n) for n in g.integers(1, 400, 10)]
    lengths[3] = 0
    clips = [_clip(n, 500 + i) for i, n in enumerate(lengths)]
    targets = ["".join(g.choice(list(CHARS), int(k))) for k in g.integers(1, 30, 10)]
    weights = [0.5, 0.2, 0.3]
    ens = EnsembleTFLiteModel(models, weights=weights, batch_size=4, max_frames=512)
    return dict(models=models, clips=clips, targets=targets, weights=weights, ens=ens, logits=ens.logits(clips))


def _resolved(ref, err):
    """the clips all of whose frames the fp64 reference decides by more than twice the error"""
    return [b for b in range(ref.shape[0]) if (frame_margins(ref[b]) > 2 * max(err, 1e-7)).all()]


def test_wrapper_logits_and_decodes(trio):
    ens, lg, clips = trio["ens"], trio["logits"], trio["clips"]
    assert lg["x"].shape == (10, 176, 276) and lg["per_model"].shape == (3, 10, 176, Cn) and lg["combined"].shape == (10, 176, Cn)
    for m, model in enumerate(trio["models"]):                # each model alone on the same input, at the batch size the wrapper ran it at
        for b0 in range(0, 10, 4):
            x = np.zeros((4, 176, 276), np.float32)
            n = min(4, 10 - b0)
            x[:n] = lg["x"][b0:b0 + n]
            own = model(torch.from_numpy(x)).cpu().numpy()[:n]
            assert np.array_equal(own.view(np.uint32), lg["per_model"][m, b0:b0 + n].view(np.uint32)), (m, b0)
    ref = combine_reference(list(lg["per_model"]), ens.weights, "log_linear")
    scale = 1.0 + np.abs(lg["per_model"]).max(axis=(0, 3)) + np.abs(ref).max(axis=-1)      # the bound of ensemble_parity.compare (no temperatures: z = logits)
    ratio = float((np.abs(lg["combined"] - ref).max(axis=-1) / (P.K * P.EPS * scale)).max())
    print(f"wrapper: combined err / bound {ratio:.4f}")
    assert ratio <= 1.0
    decodes = ens.predict_indices(clips)
    # min_frac 0.9 as the single-model wrapper's test has it: on the MI355X every frame's fp64 top-2 margin exceeds twice the fused rows' error
    # (1760 of 1760 frames, all 10 clips compared whole), so the floor is not lowered
    rec = check_decode_parity(ref, lg["combined"], decodes, O.decode_phrase, min_frac=0.9, what="ensemble vs fp64 fusion")
    print(f"wrapper: {rec['frac_compared']:.3f} of the frames resolved, {rec['clips_compared']} clips compared whole")
    eager = EnsembleTFLiteModel(trio["models"], weights=trio["weights"], batch_size=4, max_frames=512, use_graph=False)
    assert all(np.array_equal(a, b) for a, b in zip(decodes, eager.predict_indices(clips)))
    assert np.array_equal(eager.logits(clips)["combined"].view(np.uint32), lg["combined"].view(np.uint32))


def test_wrapper_of_one_model_and_one_hot_weights(trio):
    clips, lg, ens = trio["clips"], trio["logits"], trio["ens"]
    compared = 0
    ens.predict_indices(clips)
    graphs = len(ens._graphs)
    try:
        for m, model in enumerate(trio["models"]):
            alone = BatchedTFLiteModel(model, batch_size=4, max_frames=512).predict_indices(clips)
            whole = _resolved(lg["per_model"][m].astype(np.float64), 1e-5)        # 1e-5: far above the fusion's rounding of O(1) logits
            one_hot = [1.0 if k == m else 0.0 for k in range(3)]
            ens.set_weights(one_hot)                                             # no new capture: the graph of the fixture is replayed
            assert ens.weights.tolist() == one_hot
            got = ens.predict_indices(clips)
            single = EnsembleTFLiteModel([model], batch_size=4, max_frames=512).predict_indices(clips) if m == 0 else None
            for b in whole:
                assert np.array_equal(got[b], alone[b]), (m, b)
                assert single is None or np.array_equal(single[b], alone[b]), b
            compared += len(whole)
        assert len(ens._graphs) == graphs, "set_weights captured again"
    finally:
        ens.set_weights(trio["weights"])
    assert compared >= 3, "no clip was resolved as a whole"


def test_wrapper_scores(trio):
    ens, clips, targets = trio["ens"], trio["clips"], trio["targets"]
    num_to_char = {i: ch for ch, i in CHAR_TO_NUM.items()}
    preds = ["".join(num_to_char.get(int(s), "") for s in np.argmax(o["outputs"], axis=1)) for o in ens(clips)]
    res = ens.score(clips, targets, CHAR_TO_NUM)
    assert res["mean_score"] == mean_score(preds, targets)
    brk = ens.score(clips, targets, CHAR_TO_NUM, breakdown=True)
    assert brk["distances"].tolist() == res["distances"].tolist()
    assert brk["ops"][:, 1:].sum(axis=1).tolist() == res["distances"].tolist() and brk["report"] is not None
    cands = [[1, 1, 1], [0, 1, 0], [0.7, 0.0, 0.3]]
    many = ens.score_weights(clips, targets, cands, CHAR_TO_NUM)
    assert many["distances"].shape == (3, 10) and ens.weights.tolist() == pytest.approx(trio["weights"])
    try:
        for k, c in enumerate(cands):
            ens.set_weights(c)
            one = ens.score(clips, targets, CHAR_TO_NUM)
            assert one["distances"].tolist() == many["distances"][k].tolist(), k
            assert one["mean_score"] == many["mean_scores"][k]
    finally:
        ens.set_weights(trio["weights"])
    assert ens.score(clips, targets, CHAR_TO_NUM)["distances"].tolist() == res["distances"].tolist()      # score_weights left the weights alone


def test_wrapper_beam_top1_is_the_beam_decoder_on_the_fused_logits(trio):
    g = np.random.default_rng(3)
    lm = CharBigramLM.fit([g.integers(0, BLANK, int(g.integers(3, 20))).tolist() for _ in range(200)], num_classes=Cn, smoothing=0.5)
    ens = EnsembleTFLiteModel(trio["models"], weights=trio["weights"], mode="linear", temperatures=[1.0, 0.8, 1.25], batch_size=4, max_frames=512,
                              beam_width=4, lm=lm, lm_alpha=0.3, lm_beta=0.2)
    clips = trio["clips"]
    got = ens.predict_indices(clips)
    lg = ens.logits(clips)
    fused = lg["combined"]
    ref = combine_reference(list(lg["per_model"]), ens.weights, "linear", [1.0, 0.8, 1.25])
    assert np.abs(fused - ref).max() < 1e-4
    want = ctc_beam_decode(torch.from_numpy(fused).cuda(), beam_width=4, lm=lm, alpha=0.3, beta=0.2)
    assert [g_.tolist() for g_ in got] == [w[0][0].tolist() for w in want]
