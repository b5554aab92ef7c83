"""GPU: ishara_mbr_select (csrc/mbr_select.hip) over the case table of tests/mbr_parity.py (exact distances, selection and status; risk
bit-equal to the float32 recomputation from the device's own votes; votes within the derived bound), its contract (every output written,
optional outputs, 4-byte alignment, determinism, graph replay with a rewritten temperature and rewritten weights), and the chain: the beam
search's n-best -> the selection, Model.mbr_decode, the TFLite-shaped wrappers with mbr_nbest, and pool_nbest across models of different T."""
import numpy as np
import pytest
import torch

import mbr_parity as P
from ishara_amd import _lib, get_model, mbr
from ishara_amd.ctc import ctc_beam_nbest_device
from ishara_amd.ensemble import EnsembleTFLiteModel
from ishara_amd.evaluation import mean_score
from ishara_amd.tflite_batch import BatchedTFLiteModel, apply_fallback
from ishara_amd.tflite_model import TFLiteModel

pytestmark = pytest.mark.gpu

CHARS = " !#$%&'()*+,-./0123456789:;=?@[_abcdefghijklmnopqrstuvwxyz~"
CHAR_TO_NUM = {c: i for i, c in enumerate(CHARS)}
Cn, BLANK = 60, 59
SMALL = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276))
CASES = {c["name"]: c for c in P.cases()}
OUTS = ("out_idx", "out_len", "best", "risk", "w_out", "dist", "status")


def _dev(a, offset=0):
    """a numpy array on the device, `offset` elements into its allocation (offset 1: an address that is 4-byte aligned and no more)"""
    a = np.array(a)
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = buf[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert offset == 0 or a.size == 0 or view.data_ptr() % 8 == 4
    return view


def _buffers(case, offset=0):
    """the inputs on the device and every output poisoned: NaN in the float outputs, -77 in the integer ones (-1 is a value they take)"""
    B, N, T = case["B"], case["N"], case["T"]
    ins = dict(hyp_idx=_dev(case["hyp_idx"], offset), hyp_len=_dev(case["hyp_len"], offset),
               hyp_score=None if case["hyp_score"] is None else _dev(case["hyp_score"], offset),
               weights=None if case["weights"] is None else _dev(case["weights"], offset),
               inv_temp=None if case["inv_temp"] is None else _dev(np.array([case["inv_temp"]], np.float32), offset))
    outs = dict(out_idx=_dev(np.full((B, T), -77, np.int32), offset), out_len=_dev(np.full(B, -77, np.int32), offset), best=_dev(np.full(B, -77, np.int32), offset),
                risk=_dev(np.full((B, N), np.nan, np.float32), offset), w_out=_dev(np.full((B, N), np.nan, np.float32), offset),
                dist=_dev(np.full((B, N, N), -77, np.int32), offset), status=_dev(np.full(B, -77, np.int32), offset))
    return ins, outs


def _launch(lib, case, ins, outs, optional=True):
    o = {k: (outs[k] if optional or k in OUTS[:3] else None) for k in OUTS}
    mbr.launch(lib, ins["hyp_idx"], ins["hyp_len"], ins["hyp_score"], ins["weights"], ins["inv_temp"], case["B"], case["N"], case["T"], case["C"],
               case["mode"], o["out_idx"], o["out_len"], o["best"], o["risk"], o["w_out"], o["dist"], o["status"], _lib.stream())


def _run(lib, case, offset=0, optional=True):
    ins, outs = _buffers(case, offset)
    _launch(lib, case, ins, outs, optional)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def _bits(res):
    return [res[k].view(np.uint32) if res[k].dtype == np.float32 else res[k] for k in OUTS]


# ------------------------------------------------------------------------------------------------ 1. the operator
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_reference(lib, name):
    """every output of a poisoned set is written; dist, best, out_idx, out_len and status equal the reference's; risk equals the float32
    recomputation from the device's w_out in every bit; w_out lies within the bound of the fp64 votes"""
    case = CASES[name]
    got = _run(lib, case)
    fails, ratio = P.check(case, got)
    print(f"{name}: w_out err / bound {ratio:.4f} (K = {P.K}); best {got['best'][:8].tolist()}")
    assert not fails, fails[:4]
    assert not np.isnan(got["w_out"]).any() and (got["out_idx"] != -77).all() and (got["dist"] != -77).all()


def test_an_empty_batch_is_a_no_op(lib):
    case = dict(CASES[sorted(CASES)[0]], B=0)
    ins, outs = _buffers(CASES[sorted(CASES)[0]])
    _launch(lib, case, ins, outs)
    torch.cuda.synchronize()
    assert (outs["best"] == -77).all() and (outs["out_idx"] == -77).all()


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n]["N"] in (3, 33, 64)][:6])
def test_optional_outputs_and_alignment(lib, name):
    case = CASES[name]
    full = _run(lib, case)
    bare = _run(lib, case, optional=False)                # risk, w_out, dist and status passed as NULL
    for k in OUTS[:3]:
        assert np.array_equal(bare[k], full[k]), k
    assert np.isnan(bare["risk"]).all() and (bare["dist"] == -77).all() and (bare["status"] == -77).all()       # untouched
    odd = _run(lib, case, offset=1)                       # every buffer 4-byte aligned and no more
    assert all(np.array_equal(a, b) for a, b in zip(_bits(odd), _bits(full))), "the result depends on the buffers' alignment"


def test_two_runs_are_bit_identical(lib):
    for name in sorted(CASES)[::5]:
        a, b = _run(lib, CASES[name]), _run(lib, CASES[name])
        assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b))), name


@pytest.mark.parametrize("votes", ["scores", "weights"])
def test_graph_replay_reads_the_rewritten_temperature_and_weights(lib, votes):
    base = next(c for c in P.cases() if c["N"] == 32 and c["mode"] == 1)
    g = np.random.default_rng(41)
    sc = -np.sort(g.random((base["B"], base["N"])) * 5, axis=1).astype(np.float32)
    w0 = g.random((base["B"], base["N"])).astype(np.float32)
    case = dict(base, hyp_score=sc, weights=w0 if votes == "weights" else None, inv_temp=np.float32(1.0), adhoc=True, name="graph")
    ins, outs = _buffers(case)
    _launch(lib, case, ins, outs)                         # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(lib, case, ins, outs)
    graph.replay()
    first = {k: v.cpu().numpy() for k, v in outs.items()}
    assert not P.check(case, first)[0]
    if votes == "weights":
        w1 = (w0[:, ::-1] ** 4).copy()
        ins["weights"].copy_(torch.from_numpy(w1))
        case = dict(case, weights=w1)
    else:
        ins["inv_temp"].fill_(8.0)
        case = dict(case, inv_temp=np.float32(8.0))
    for v in outs.values():
        v.fill_(float("nan") if v.dtype == torch.float32 else -77)
    graph.replay()
    second = {k: v.cpu().numpy() for k, v in outs.items()}
    fails, _ = P.check(case, second)
    assert not fails, fails[:3]
    assert not np.array_equal(second["risk"].view(np.uint32), first["risk"].view(np.uint32)), "the replay did not read the rewritten values"


# ------------------------------------------------------------------------------------------------ 2. the chain
def _synthetic(seed, B, T, sharp=3.0, noise=1.8):
    """noisy confident alignments: logits whose n-best lists hold several distinct, similar hypotheses"""
    g = np.random.default_rng(seed)
    x = np.zeros((B, T, Cn))
    for b in range(B):
        t, prev = 0, None
        while t < T - 4:
            n = int(g.integers(2, 5))
            c = BLANK if (prev not in (None, BLANK) and g.random() < 0.5) else int(g.integers(0, BLANK))
            x[b, t:min(t + n, T - 4), BLANK if c == prev else c] += sharp
            prev, t = c, t + n
        x[b, T - 4:, BLANK] += sharp
    return (x + noise * g.standard_normal(x.shape)).astype(np.float32)


def _select_and_check(name, hyp, inv_temp, mode, C=Cn):
    """mbr_select on device n-best tensors, checked against the reference on those same tensors; returns the decodes"""
    idx, ln, best, det = mbr.mbr_select(*hyp, inv_temp=inv_temp, mode=mode, C=C, return_details=True)
    case = P.adhoc_case(name, hyp[0].cpu().numpy(), hyp[1].cpu().numpy(), hyp[2].cpu().numpy(), C, mode, inv_temp)
    got = dict(out_idx=idx.cpu().numpy(), out_len=ln.cpu().numpy(), best=best.cpu().numpy(), risk=det["risk"].cpu().numpy(), w_out=det["votes"].cpu().numpy(),
               dist=det["dist"].cpu().numpy(), status=det["status"].cpu().numpy())
    fails, ratio = P.check(case, got)
    assert not fails, (name, fails[:3])
    return [got["out_idx"][b, :got["out_len"][b]].astype(np.int64) for b in range(case["B"])], got


def test_beam_nbest_then_selection_equals_the_reference():
    x = torch.from_numpy(_synthetic(3, 12, 64)).cuda()
    moved = 0
    for mode, temp in ((0, 4.0), (1, 8.0)):
        hyp = ctc_beam_nbest_device(x, beam_width=16, nbest=8)
        assert hyp[0].shape == (12, 8, 64) and hyp[0].dtype == torch.int32 and hyp[2].dtype == torch.float32
        decodes, got = _select_and_check(f"chain-mode{mode}", hyp, mbr.inverse_temperature(temp), mode)
        moved += int((got["best"] > 0).sum())
        lens = ctc_beam_nbest_device(x, [64, 40] * 6, beam_width=16, nbest=8)          # per-clip frame counts reach the search
        assert not torch.equal(lens[0], hyp[0])
    print(f"the selection left the beam's top-1 in {moved} of 24 clips")
    assert moved > 0


def test_model_mbr_decode(lib):
    model = get_model(**SMALL, dtype="f32", max_batch=4, seed=5)
    x = torch.from_numpy(_synthetic(4, 4, 64)).cuda()
    res = model.mbr_decode(x, beam_width=8, nbest=4, temperature=6.0, normalise=True)
    hyp = ctc_beam_nbest_device(x, beam_width=8, nbest=4)
    decodes, got = _select_and_check("model", hyp, mbr.inverse_temperature(6.0), 1)
    for b, (ind, slot, risk) in enumerate(res):
        assert np.array_equal(ind, decodes[b]) and slot == got["best"][b] and np.float32(risk) == got["risk"][b, slot]
    with pytest.raises(ValueError):
        model.mbr_decode(x, beam_width=4, nbest=8)
    with pytest.raises(ValueError):
        model.mbr_decode(x, temperature=0.0)


def _clip(n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, 276)).astype(np.float32)
    x[g.random(n) < 0.3, :42] = np.nan
    return x


@pytest.fixture(scope="module")
def small():
    model = get_model(**SMALL, dtype="f32", max_batch=4, seed=5)
    g = np.random.default_rng(12)
    clips = [_clip(int(n), 700 + i) for i, n in enumerate(g.integers(1, 400, 7))]
    targets = ["".join(g.choice(list(CHARS), int(k))) for k in g.integers(1, 30, 7)]
    return dict(model=model, clips=clips, targets=targets)


def _chain_of_wrapper(bm, clips, temp, name):
    """the wrapper's batches one at a time: its decode, and the chain beam n-best -> selection on the logits it left on the device"""
    got, want = [], []
    for b0 in range(0, len(clips), bm.batch_size):
        part = clips[b0:b0 + bm.batch_size]
        got.extend(bm.predict_indices(part))
        hyp = ctc_beam_nbest_device(bm._logits[:len(part)].clone(), beam_width=8, nbest=4)
        want.extend(_select_and_check(f"{name}-{b0}", hyp, mbr.inverse_temperature(temp), 1)[0])
    return got, want


def test_batched_wrapper_decodes_and_scores_the_mbr_choice(small):
    model, clips, targets = small["model"], small["clips"], small["targets"]
    bm = BatchedTFLiteModel(model, batch_size=4, max_frames=512, beam_width=8, mbr_nbest=4, mbr_temperature=20.0)
    got, want = _chain_of_wrapper(bm, clips, 20.0, "batched")
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    num_to_char = {i: ch for ch, i in CHAR_TO_NUM.items()}
    preds = ["".join(num_to_char.get(int(s), "") for s in apply_fallback(w)) for w in want]
    res = bm.score(clips, targets, CHAR_TO_NUM)
    assert res["mean_score"] == mean_score(preds, targets)
    brk = bm.score(clips, targets, CHAR_TO_NUM, breakdown=True)
    assert brk["distances"].tolist() == res["distances"].tolist() and brk["ops"][:, 1:].sum(axis=1).tolist() == res["distances"].tolist()
    # the temperature lives on the device: no new capture, and the replay follows it
    bm.predict_indices(clips)                             # both staging slots have their decode graph now
    graphs = len(bm._graphs)
    bm.set_mbr_temperature(0.05)
    sharp = bm.predict_indices(clips)
    assert len(bm._graphs) == graphs, "set_mbr_temperature captured again"
    fresh = BatchedTFLiteModel(model, batch_size=4, max_frames=512, beam_width=8, mbr_nbest=4, mbr_temperature=0.05, use_graph=False)
    assert all(np.array_equal(a, b) for a, b in zip(sharp, fresh.predict_indices(clips)))
    # the single-clip wrapper: the same chain on its own logits (B = 1)
    one = TFLiteModel(model, max_frames=512, beam_width=8, mbr_nbest=4, mbr_temperature=20.0)
    for k, c in enumerate(clips[:3]):
        ind = one.predict_indices(c)
        hyp = ctc_beam_nbest_device(one._logits.clone(), beam_width=8, nbest=4)
        assert np.array_equal(ind, _select_and_check(f"single-{k}", hyp, mbr.inverse_temperature(20.0), 1)[0][0])
    for kw in (dict(beam_width=2, mbr_nbest=4), dict(beam_width=0, mbr_nbest=2), dict(beam_width=8, mbr_nbest=1), dict(beam_width=8, mbr_nbest=4, mbr_temperature=0)):
        with pytest.raises(ValueError):
            BatchedTFLiteModel(model, batch_size=4, max_frames=512, **kw)


def test_mbr_off_is_the_plain_beam_wrapper(small):
    model, clips, targets = small["model"], small["clips"], small["targets"]
    plain = BatchedTFLiteModel(model, batch_size=4, max_frames=512, beam_width=8)
    off = BatchedTFLiteModel(model, batch_size=4, max_frames=512, beam_width=8, mbr_nbest=0, mbr_temperature=3.0, mbr_normalise=False)
    assert off._mbr is None and plain._mbr is None
    a, b = plain.predict_indices(clips), off.predict_indices(clips)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    ra, rb = plain.score(clips, targets, CHAR_TO_NUM), off.score(clips, targets, CHAR_TO_NUM)
    assert ra["mean_score"] == rb["mean_score"] and ra["distances"].tolist() == rb["distances"].tolist()
    with pytest.raises(ValueError):
        off.set_mbr_temperature(2.0)


def test_ensemble_wrapper_with_mbr(small):
    models = [small["model"], get_model(**SMALL, dtype="bf16", max_batch=4, seed=6)]
    ens = EnsembleTFLiteModel(models, weights=[0.6, 0.4], batch_size=4, max_frames=512, beam_width=8, mbr_nbest=4, mbr_temperature=20.0)
    got, want = _chain_of_wrapper(ens, small["clips"], 20.0, "ensemble")
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_pool_nbest_of_two_models_with_different_T():
    a = ctc_beam_nbest_device(torch.from_numpy(_synthetic(8, 5, 64)).cuda(), beam_width=8, nbest=4)
    b = ctc_beam_nbest_device(torch.from_numpy(_synthetic(9, 5, 48)).cuda(), beam_width=8, nbest=6)
    pooled = mbr.pool_nbest([a, b], model_weights=[0.7, 0.3])
    assert pooled[0].shape == (5, 10, 64) and (pooled[0][:, 4:, 48:] == -1).all()
    assert torch.equal(pooled[1], torch.cat([a[1], b[1]], dim=1))
    decodes, got = _select_and_check("pooled", pooled, mbr.inverse_temperature(6.0), 1)
    assert (got["status"] == 0).all() and len(decodes) == 5
    with pytest.raises(ValueError):
        mbr.pool_nbest([a, (b[0].cpu(), b[1].cpu(), b[2].cpu())])


def test_device_side_refusals():
    idx = torch.zeros((2, 3, 5), dtype=torch.int32, device="cuda")
    ln = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    sc = torch.zeros((2, 3), device="cuda")
    mbr.mbr_select(idx, ln, sc)
    for args, kw in (((idx.long(), ln, sc), {}), ((idx[0], ln, sc), {}), ((idx, ln[:1], sc), {}), ((idx, ln.float(), sc), {}), ((idx, ln, sc.double()), {}),
                     ((idx, ln, None), {}), ((idx, ln, sc), dict(weights=sc[:, :2])), ((idx, ln, sc), dict(inv_temp=0.0)), ((idx, ln, sc), dict(inv_temp=float("nan"))),
                     ((idx, ln, sc), dict(inv_temp=torch.ones(2, device="cuda"))), ((idx, ln, sc), dict(inv_temp=torch.ones(1))), ((idx, ln, sc), dict(mode=2)),
                     ((idx, ln, sc), dict(C=65)), ((idx, ln.cpu(), sc), {}), ((torch.zeros((1, 65, 2), dtype=torch.int32, device="cuda"), ln, sc), {})):
        with pytest.raises(ValueError):
            mbr.mbr_select(*args, **kw)
    with pytest.raises(ValueError):
        ctc_beam_nbest_device(torch.zeros((1, 8, Cn), device="cuda"), beam_width=4, nbest=8)
    with pytest.raises(_lib.IsharaError):
        ctc_beam_nbest_device(torch.zeros((1, 8, Cn)), beam_width=8, nbest=4)
