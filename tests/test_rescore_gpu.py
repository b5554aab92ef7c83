"""GPU: ishara_ctc_score_nbest (csrc/ctc_score.hip) and ishara_nbest_rescore (csrc/nbest_rescore.hip) over the cases of tests/rescore_parity.py.
  score     bit-equal to float32(-nll) of ishara_ctc_loss_ex for every scored slot, within the loss's own bound of the fp64 forward algorithm,
            status and isolation of the slots it does not score, rows past a clip's end never read, the same bits under every
            slot-to-wave mapping
  rescore   out_score in every bit, order, perm, dedupe and the dead-slot layout equal to rescore_reference fed the device's own logp_m;
            the posterior within the derived bound
  chain     the beam search without pruning scores exactly; rescore_models across two models of different T, accepted by mbr_select;
            Model.rescore_decode; determinism; both calls in one captured graph that follows rewritten weights and temperature"""
import numpy as np
import pytest
import torch

import rescore_parity as P
from ishara_amd import _lib, get_model, mbr, rescore
from ishara_amd.ctc import ctc_beam_nbest_device

pytestmark = pytest.mark.gpu

SCORE = {c["name"]: c for c in P.score_cases()}
RESCORE = {c["name"]: c for c in P.rescore_cases()}
SMALL = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276))


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the cases' arrays are read-only


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _score(case):
    fl = None if case["frame_len"] is None else _dev(case["frame_len"])      # a device tensor is handed on unchecked: 0 and T + 1 reach the kernel
    logp, st = rescore.ctc_score_nbest(_dev(case["logits"]), _dev(case["hyp_idx"]), _dev(case["hyp_len"]), fl, case["blank"], return_status=True)
    return logp.cpu().numpy(), st.cpu().numpy()


def _loss_logp(lib, case, want):
    """float32(-nll) [B, N] of ishara_ctc_loss_ex, one launch per slot: the clip's hypothesis n, padded with blank, as its label row (an
    empty row where the slot is not scored), the same frame_len"""
    B, N, T, Cn, bl = case["B"], case["N"], case["T"], case["C"], case["blank"]
    ok = want == 0
    L = max(int(np.where(ok, case["hyp_len"], 0).max()), 1)
    x = _dev(case["logits"])
    fl = None if case["frame_len"] is None else _dev(case["frame_len"])
    ws = torch.empty(int(lib.ishara_ctc_workspace_bytes(B, T, L)), dtype=torch.uint8, device="cuda")
    out = np.zeros((B, N), np.float32)
    for n in range(N):
        y = np.full((B, L), bl, np.int64)
        for b in range(B):
            if ok[b, n]:
                y[b, :case["hyp_len"][b, n]] = case["hyp_idx"][b, n, :case["hyp_len"][b, n]]
        nll = torch.empty(B, dtype=torch.float32, device="cuda")
        _lib.check(lib.ishara_ctc_loss_ex(_lib.ptr(x), _lib.ptr(_dev(y)), B, T, Cn, L, bl, _lib.ptr(nll), None, _lib.C.c_float(1.0), _lib.ptr(ws), _lib.ptr(fl),
                                          None, 0, _lib.stream()), "ishara_ctc_loss_ex")
        out[:, n] = -nll.cpu().numpy()
    return out


# ------------------------------------------------------------------------------------------------ 1. the exact scores
@pytest.mark.parametrize("name", sorted(SCORE))
def test_score_equals_the_loss_bit_for_bit_and_the_fp64_reference(lib, name):
    case = SCORE[name]
    logp, st = _score(case)
    fails, ratio = P.check_score(case, logp, st)
    print(f"{name}: logp err / bound {ratio:.4g}")
    assert not fails, fails[:3]
    want = P.expected_status(case)
    loss = _loss_logp(lib, case, want)
    ok = want == 0
    assert ok.any() and np.array_equal(_bits(logp[ok]), _bits(loss[ok])), (logp[ok] - loss[ok]).tolist()


def test_status_and_isolation_of_bad_slots(lib):
    bad, removed, want = P.bad_slot_case()
    a, sa = _score(bad)
    b, sb = _score(removed)
    assert np.array_equal(sa, want), sa.tolist()
    assert np.isneginf(a[want != 0]).all() and np.isfinite(a[want == 0]).all()
    assert np.array_equal(_bits(a[want == 0]), _bits(b[want == 0])), "a bad slot changed its neighbours' bits"
    assert not P.check_score(bad, a, sa, P.score_reference_of(bad))[0]
    loss = _loss_logp(lib, bad, want)
    assert np.array_equal(_bits(a[want == 0]), _bits(loss[want == 0]))


def test_the_slot_to_wave_mapping_does_not_change_a_bit(lib):
    try:
        for name in ("N64", "seams", "ragged-long"):
            lib.ishara_debug_set_score_group(0)
            base = _score(SCORE[name])
            for hpw in (1, 2, 3, 16):
                lib.ishara_debug_set_score_group(hpw)
                got = _score(SCORE[name])
                assert np.array_equal(_bits(got[0]), _bits(base[0])) and np.array_equal(got[1], base[1]), (name, hpw)
    finally:
        lib.ishara_debug_set_score_group(0)


def test_status_is_optional_and_an_empty_batch_is_a_no_op(lib):
    case = SCORE["tight"]
    full = _score(case)[0]
    bare = rescore.ctc_score_nbest(_dev(case["logits"]), _dev(case["hyp_idx"]), _dev(case["hyp_len"]), _dev(case["frame_len"]), case["blank"]).cpu().numpy()
    assert np.array_equal(_bits(full), _bits(bare))
    logp = torch.full((2, 3), 7.0, device="cuda")
    z = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert lib.ishara_ctc_score_nbest(_lib.ptr(logp), 0, 4, 8, 7, _lib.ptr(z), _lib.ptr(z), 3, 4, None, _lib.ptr(logp), None, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert (logp == 7.0).all()


# ------------------------------------------------------------------------------------------------ 2. combine, dedupe, rerank
def _device_logps(case):
    """the device's own per-model scores: a list of M tensors [B, N] (NaN where the model must not be read) and the same as float32 [M, B, N]"""
    idx, ln = _dev(case["hyp_idx"]), _dev(case["hyp_len"])
    out = []
    for m in range(case["M"]):
        if m in case["nan_models"]:
            out.append(torch.full((case["B"], case["N"]), float("nan"), device="cuda"))
        else:
            out.append(rescore.ctc_score_nbest(_dev(case["logits"][m]), idx, ln, None, case["blank"]))
    return out, np.stack([t.cpu().numpy() for t in out])


def _rescore_buffers(case):
    B, N, Th = case["B"], case["N"], case["Th"]
    return dict(out_idx=_dev(np.full((B, N, Th), -77, np.int32)), out_len=_dev(np.full((B, N), -77, np.int32)), out_score=_dev(np.full((B, N), np.nan, np.float32)),
                posterior=_dev(np.full((B, N), np.nan, np.float32)), perm=_dev(np.full((B, N), -77, np.int32)))


def _rescore_launch(lib, case, idx, ln, logps, w_d, it_d, lm_dev, outs, optional=True):
    rescore.launch(lib, idx, ln, case["B"], case["N"], case["Th"], rescore.pointer_array(logps), case["M"], w_d, lm_dev, case["blank"], case["alpha"], case["beta"],
                   it_d, outs["out_idx"], outs["out_len"], outs["out_score"], outs["posterior"] if optional else None, outs["perm"] if optional else None,
                   _lib.stream())


def _rescore_inputs(case):
    w_d = _dev(case["weights"])
    it_d = None if case["inv_temp"] is None else _dev(np.array([case["inv_temp"]], np.float32))
    return _dev(case["hyp_idx"]), _dev(case["hyp_len"]), w_d, it_d, rescore.lm_to_device(case["lm"], "cuda", case["blank"])


@pytest.mark.parametrize("name", sorted(RESCORE))
def test_rescore_equals_the_reference(lib, name):
    """every output of a poisoned set is written; score bits, order, perm, dedupe and dead-slot layout equal the reference fed the device's
    own logp_m; the posterior lies within the derived bound"""
    case = RESCORE[name]
    logps, lp = _device_logps(case)
    for m in range(case["M"]):                               # the device's scores are themselves within the loss's bound of fp64
        if m not in case["nan_models"]:
            sc = P.model_score_case(case, m)
            assert not P.check_score(sc, lp[m], None, P.score_reference_of(sc))[0]
    idx, ln, w_d, it_d, lm_dev = _rescore_inputs(case)
    outs = _rescore_buffers(case)
    _rescore_launch(lib, case, idx, ln, logps, w_d, it_d, lm_dev, outs)
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    fails, ratio = P.check_rescore(case, got, lp)
    print(f"{name}: posterior err / bound {ratio:.4f}")
    assert not fails, fails[:3]
    assert (got["out_idx"] != -77).all() and (got["out_len"] != -77).all() and (got["perm"] != -77).all()
    assert not np.isnan(got["posterior"]).any()
    bare = _rescore_buffers(case)                            # posterior and perm passed as NULL: the rest has the same bits, the two stay untouched
    _rescore_launch(lib, case, idx, ln, logps, w_d, it_d, lm_dev, bare, optional=False)
    assert torch.equal(bare["out_idx"], outs["out_idx"]) and torch.equal(bare["out_len"], outs["out_len"])
    assert np.array_equal(_bits(bare["out_score"].cpu().numpy()), _bits(got["out_score"]))
    assert torch.isnan(bare["posterior"]).all() and (bare["perm"] == -77).all()
    # the public wrapper gives the same tensors
    pub = rescore.rescore_nbest(idx, ln, logps, w_d, case["lm"], case["alpha"], case["beta"],
                                it_d if it_d is not None else 1.0, return_details=True, blank=case["blank"])
    assert torch.equal(pub[0], outs["out_idx"]) and torch.equal(pub[1], outs["out_len"]) and torch.equal(pub[3]["perm"], outs["perm"])
    assert np.array_equal(_bits(pub[2].cpu().numpy()), _bits(got["out_score"])) and np.array_equal(_bits(pub[3]["posterior"].cpu().numpy()), _bits(got["posterior"]))


# ------------------------------------------------------------------------------------------------ 3. the chain
def test_a_beam_that_prunes_nothing_scores_exactly():
    """C 3, T 4, W 32: at most 31 strings, the beam search drops none, so its out_score is the whole forward sum"""
    g = np.random.default_rng(80)
    x = (g.standard_normal((4, 4, 3)) * np.array([1.0, 2.0, 2.0, 6.0])[:, None, None]).astype(np.float32)
    idx, ln, sc = ctc_beam_nbest_device(_dev(x), None, 32, 32)
    logp, st = rescore.ctc_score_nbest(_dev(x), idx, ln, return_status=True)
    idx, ln, sc, logp, st = (t.cpu().numpy() for t in (idx, ln, sc, logp, st))
    live = ln >= 0
    assert (live.sum(1) == 15).all() and (st[live] == 0).all() and (st[~live] == rescore.STATUS_DEAD).all()
    worst = 0.0
    for b in range(4):
        for n in np.nonzero(live[b])[0]:
            ref = rescore.ctc_logp_reference(x[b], idx[b, n, :ln[b, n]], 2)
            bound = P.NLL_ATOL + P.NLL_RTOL * abs(ref)
            worst = max(worst, abs(float(sc[b, n]) - float(logp[b, n])) / bound, abs(float(logp[b, n]) - ref) / bound)
    print(f"beam score vs exact score, exact score vs fp64: worst err / bound {worst:.4g}")
    assert worst <= 1.0


def _two_models():
    """two models of different T over the same clips: the second sees a time-stretched, noisier copy, so the two n-best lists share strings"""
    g = np.random.default_rng(81)
    B, Cn = 3, 8
    a = np.zeros((B, 12, Cn))
    for b in range(B):
        for t in range(12):
            a[b, t, int(g.integers(0, Cn))] += 4.0
    a += g.standard_normal(a.shape)
    bb = a[:, (np.arange(20) * 12) // 20] + 0.7 * g.standard_normal((B, 20, Cn))
    return a.astype(np.float32), bb.astype(np.float32)


def test_rescore_models_pools_two_models_of_different_T(lib):
    xa, xb = _two_models()
    da, db = _dev(xa), _dev(xb)
    la, lb = ctc_beam_nbest_device(da, None, 8, 4), ctc_beam_nbest_device(db, [20, 17, 20], 8, 4)
    pooled = mbr.pool_nbest([la, lb])
    assert pooled[0].shape == (3, 8, 20)
    idx, ln, sc, det = rescore.rescore_models([da, db], [None, [20, 17, 20]], pooled, model_weights=[0.6, 0.4], beta=0.2, temperature=2.0, return_details=True)
    hyp_idx, hyp_len = pooled[0].cpu().numpy(), pooled[1].cpu().numpy()
    lp = np.stack([t.cpu().numpy() for t in det["logps"]])
    for m, (x, fl) in enumerate(((xa, None), (xb, np.array([20, 17, 20], np.int32)))):
        sc_case = dict(name=f"pooled-{m}", logits=x, blank=7, hyp_idx=hyp_idx, hyp_len=hyp_len, frame_len=fl, B=3, T=x.shape[1], C=8, N=8, Th=20)
        assert not P.check_score(sc_case, lp[m], None, P.score_reference_of(sc_case))[0]
    case = dict(name="pooled", hyp_idx=hyp_idx, hyp_len=hyp_len, weights=np.array([0.6, 0.4], np.float32), lm=None, alpha=0.0, beta=0.2,
                inv_temp=np.float32(mbr.inverse_temperature(2.0)), C=8, blank=7, B=3, N=8, Th=20, M=2)
    got = dict(out_idx=idx.cpu().numpy(), out_len=ln.cpu().numpy(), out_score=sc.cpu().numpy(), posterior=det["posterior"].cpu().numpy(), perm=det["perm"].cpu().numpy())
    fails, ratio = P.check_rescore(case, got, lp)
    assert not fails, fails[:3]
    merged = int(((hyp_len >= 0).sum() - (got["out_len"] >= 0).sum()))
    print(f"pooled: {merged} duplicate slots merged, posterior err / bound {ratio:.4f}")
    assert merged >= 1, "the two models share no string: the case does not exercise the merge"
    # the result goes into the selection as it is, voted with the posterior
    oi, ol, best, d = mbr.mbr_select(idx, ln, weights=det["posterior"], mode=1, C=8, return_details=True)
    lists = mbr.nbest_to_lists(got["out_idx"], got["out_len"])
    for b in range(3):
        want, _, _, status = mbr.mbr_reference(lists[b], mode=1, C=8, votes=d["votes"][b].cpu().numpy())
        assert status == 0 and int(d["status"][b]) == 0 and int(best[b]) == want
        assert np.array_equal(_bits(d["votes"][b].cpu().numpy()), _bits(got["posterior"][b]))


def test_model_rescore_decode():
    model = get_model(**SMALL, dtype="f32", max_batch=4, seed=5)
    xa, _ = _two_models()
    x = np.concatenate([xa, np.full((3, 12, 52), -30.0, np.float32)], axis=2)      # 60 classes, the last is the blank
    x[:, :, [7, 59]] = x[:, :, [59, 7]]
    lm = P.ngram4()
    with pytest.raises(ValueError):
        model.rescore_decode(x, lm=lm)                       # an 8-class LM on 60-class logits
    res = model.rescore_decode(x, beam_width=8, nbest=4, beta=0.3)
    voted = model.rescore_decode(x, beam_width=8, nbest=4, beta=0.3, mbr=True)
    hyp = ctc_beam_nbest_device(_dev(x), None, 8, 4, None, 0.0, 0.3)      # the search takes the call's beta as well
    logp = rescore.ctc_score_nbest(_dev(x), hyp[0], hyp[1])
    idx, ln, sc, det = rescore.rescore_nbest(hyp[0], hyp[1], logp, beta=0.3, return_details=True)
    best = mbr.mbr_select(idx, ln, weights=det["posterior"], mode=1, C=60)[2].cpu().numpy()
    idx, ln, sc, post = idx.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy(), det["posterior"].cpu().numpy()
    for b in range(3):
        assert np.array_equal(res[b][0], idx[b, 0, :ln[b, 0]]) and res[b][1] == float(sc[b, 0]) and res[b][2] == float(post[b, 0])
        k = int(best[b])
        assert np.array_equal(voted[b][0], idx[b, k, :ln[b, k]]) and voted[b][1] == float(sc[b, k])


def test_two_runs_are_bit_identical_and_a_captured_graph_follows_rewritten_weights(lib):
    case = RESCORE["M3-weights-beta"]
    idx, ln, w_d, it_d, lm_dev = _rescore_inputs(case)
    xs = [_dev(x) for x in case["logits"]]
    logps = [torch.empty((case["B"], case["N"]), device="cuda") for _ in xs]
    outs = _rescore_buffers(case)

    def both():
        for x, lp in zip(xs, logps):
            _lib.check(lib.ishara_ctc_score_nbest(_lib.ptr(x), case["B"], x.shape[1], case["C"], case["blank"], _lib.ptr(idx), _lib.ptr(ln), case["N"], case["Th"],
                                                  None, _lib.ptr(lp), None, _lib.stream()), "ishara_ctc_score_nbest")
        _rescore_launch(lib, case, idx, ln, logps, w_d, it_d, lm_dev, outs)

    def snapshot():
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in outs.items()}, np.stack([t.cpu().numpy() for t in logps])

    both()
    first, lp1 = snapshot()
    both()
    second, lp2 = snapshot()
    assert np.array_equal(_bits(lp1), _bits(lp2))
    assert all(np.array_equal(_bits(first[k]) if first[k].dtype == np.float32 else first[k], _bits(second[k]) if second[k].dtype == np.float32 else second[k])
               for k in first)
    assert not P.check_rescore(case, first, lp1)[0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # one linear capture of the M score launches and the rescoring
        both()
    for k, v in outs.items():
        v.fill_(-77 if v.dtype == torch.int32 else float("nan"))
    graph.replay()
    third, lp3 = snapshot()
    assert np.array_equal(_bits(lp3), _bits(lp1)) and np.array_equal(_bits(third["out_score"]), _bits(first["out_score"])) and np.array_equal(third["perm"], first["perm"])
    # rewritten on the device between replays, no new capture
    new_w, new_it = np.array([0.0, 2.0, 0.125], np.float32), np.float32(0.25)
    w_d.copy_(torch.from_numpy(new_w))
    it_d.copy_(torch.from_numpy(np.array([new_it])))
    graph.replay()
    fourth, lp4 = snapshot()
    changed = dict(case, weights=new_w, inv_temp=new_it)
    fails, _ = P.check_rescore(changed, fourth, lp4)
    assert not fails, fails[:3]
    assert not np.array_equal(_bits(fourth["out_score"]), _bits(first["out_score"]))
