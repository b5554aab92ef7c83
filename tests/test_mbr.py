"""CPU: the host reference of minimum-Bayes-risk decoding (ishara_amd/mbr.py) against evaluation.levenshtein and brute force, its
properties, pool_nbest on CPU tensors, and every refusal that is made before a launch."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import mbr_parity as P
from ishara_amd import mbr
from ishara_amd.evaluation import levenshtein
from ishara_amd.tflite_model import _mbr_setup, _set_mbr_temperature
from ishara_amd.tflite_stream import StreamingTFLiteModel


def _brute(a, b):
    """the edit distance by its recursive definition"""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (a[i - 1] != b[j - 1]))
    return d(len(a), len(b))


def test_distances_equal_levenshtein_and_brute_force():
    g = np.random.default_rng(0)
    seqs = [tuple(g.integers(0, 3, int(n)).tolist()) for n in g.integers(0, 9, 14)] + [(), (), (1,)]
    pw = mbr.pairwise_levenshtein(seqs)
    for i, j in itertools.product(range(len(seqs)), repeat=2):
        want = _brute(seqs[i], seqs[j])
        assert levenshtein(list(seqs[i]), list(seqs[j])) == want
        assert mbr.levenshtein_dp(seqs[i], seqs[j]) == want and pw[i, j] == want, (seqs[i], seqs[j])
    long_ = [g.integers(0, 5, int(n)).tolist() for n in (64, 63, 33, 1, 0, 64)]
    pw = mbr.pairwise_levenshtein(long_)
    assert all(pw[i, j] == levenshtein(long_[i], long_[j]) for i in range(6) for j in range(6))
    assert mbr.pairwise_levenshtein([]).shape == (0, 0) and mbr.pairwise_levenshtein([[1, 2]]).tolist() == [[0]]


def test_reference_equals_the_definition():
    g = np.random.default_rng(1)
    for mode in (0, 1):
        hyps = [g.integers(0, 4, int(n)).tolist() for n in g.integers(0, 7, 6)]
        hyps[2] = None
        s = -g.random(6) * 3
        best, risk, dist, status = mbr.mbr_reference(hyps, scores=s, inv_temp=0.5, mode=mode, C=4)
        live = [i for i, h in enumerate(hyps) if h is not None]
        s32 = s.astype(np.float32).astype(np.float64)
        w = {j: np.exp((s32[j] - max(s32[k] for k in live)) * 0.5) for j in live}
        for i in live:
            want = sum(w[j] * levenshtein(hyps[i], hyps[j]) / (max(len(hyps[j]), 1) if mode else 1) for j in live)
            assert risk[i] == pytest.approx(want, rel=1e-12, abs=1e-15)
        assert status == 0 and np.isnan(risk[2]) and (dist[2] == -1).all() and (dist[:, 2] == -1).all()
        assert best == min(live, key=lambda i: (risk[i], i))
        assert np.array_equal(dist, dist.T) and all(dist[i, i] == 0 for i in live)


def test_reference_properties():
    assert mbr.mbr_reference([[3, 1, 2]], scores=[-2.0])[0] == 0                                  # N = 1
    assert mbr.mbr_reference([None, [3]], scores=[5.0, -2.0])[0] == 1
    g = np.random.default_rng(2)
    hyps = [g.integers(0, 5, int(n)).tolist() for n in g.integers(1, 9, 7)]
    s = -g.random(7) * 4
    _, risk, dist, _ = mbr.mbr_reference(hyps, scores=s, mode=1)
    perm = g.permutation(7)
    _, risk_p, dist_p, _ = mbr.mbr_reference([hyps[k] for k in perm], scores=s[perm], mode=1)      # the voters in another order
    assert np.allclose(risk_p, risk[perm], rtol=1e-12, atol=0) and np.array_equal(dist_p, dist[np.ix_(perm, perm)])
    # ties go to the lowest slot, whatever the order
    assert mbr.mbr_reference([[0, 1], [0, 2]], weights=[1, 1])[0] == 0
    assert mbr.mbr_reference([[0, 2], [0, 1]], weights=[1, 1])[0] == 0
    best, risk, _, _ = mbr.mbr_reference([[0, 1, 2], [0, 1, 3], [0, 1, 3]], weights=[1, 1, 1])
    assert best == 1 and risk.tolist() == [2.0, 1.0, 1.0]                                         # not the top-1
    assert mbr.mbr_reference([[0, 1, 2], [0, 1, 3], [0, 1, 3]], scores=[0.0, -9.0, -9.0])[0] == 0    # a confident top-1 keeps its place
    assert mbr.mbr_reference([[0], [1]], weights=[0, 0])[0] == 0
    # status: not ranked, the lowest live slot
    best, risk, dist, status = mbr.mbr_reference([None, [0] * 65, [0]], scores=[0, 0, 0])
    assert (best, status) == (1, mbr.STATUS_LONG) and np.isnan(risk).all() and (dist == -1).all()
    assert mbr.mbr_reference([[0, 60]], scores=[0])[3] == mbr.STATUS_SYMBOL and mbr.mbr_reference([[0, -7]], scores=[0])[3] == mbr.STATUS_SYMBOL
    assert mbr.mbr_reference([[0, 59]], scores=[0])[3] == 0 and mbr.mbr_reference([[0, 59]], scores=[0], C=59)[3] == mbr.STATUS_SYMBOL
    assert mbr.mbr_reference([None, None], scores=[0, 0])[::3] == (-1, mbr.STATUS_EMPTY)
    # votes= : the device's float32 order
    v = np.array([0.3, 0.7, 0.1], np.float32)
    _, r32, _, _ = mbr.mbr_reference([[0, 1, 2], [0, 1], [5]], mode=1, votes=v)
    f = np.float32
    assert r32.dtype == np.float32 and r32[0] == f(f(f(0) + f(v[0] * f(0))) + f(v[1] * f(f(1) / f(2)))) + f(v[2] * f(f(3) / f(1)))


def test_the_twin_passes_every_case_on_the_cpu():
    for c in P.cases():
        fails, ratio = P.check(c, P.twin(c))
        assert not fails, (c["name"], fails[:3])
    picked = [c["name"] for c in P.cases() if (P.twin(c)["best"] > 0).any()]
    assert any("handmade" in n for n in picked) and len(picked) >= 8, picked          # MBR moves away from the top-1 in many cases


def test_pool_nbest_on_cpu_tensors():
    a = (torch.tensor([[[1, 2, -1], [3, -1, -1]]], dtype=torch.int32), torch.tensor([[2, 1]], dtype=torch.int32), torch.tensor([[-1.0, -2.0]]))
    b = (torch.tensor([[[4, 5, 6, 7, 8]]], dtype=torch.int32), torch.tensor([[5]], dtype=torch.int32), torch.tensor([[-0.5]]))
    dead = (torch.full((1, 1, 2), -1, dtype=torch.int32), torch.tensor([[-1]], dtype=torch.int32), torch.tensor([[-np.inf]], dtype=torch.float32))
    idx, ln, sc = mbr.pool_nbest([a, b, dead], model_weights=[1.0, 0.5, 2.0])
    assert idx.shape == (1, 4, 5) and idx.dtype == torch.int32
    assert idx[0].tolist() == [[1, 2, -1, -1, -1], [3, -1, -1, -1, -1], [4, 5, 6, 7, 8], [-1] * 5]
    assert ln.tolist() == [[2, 1, 5, -1]]
    assert sc[0, :2].tolist() == [-1.0, -2.0] and sc[0, 2].item() == pytest.approx(-0.5 + np.log(0.5)) and sc[0, 3].item() == -np.inf
    plain = mbr.pool_nbest([a, b])
    assert plain[2].tolist() == [[-1.0, -2.0, -0.5]]
    lists = mbr.nbest_to_lists(idx.numpy(), ln.numpy())
    assert lists == [[[1, 2], [3], [4, 5, 6, 7, 8], None]]
    wide = (torch.zeros((1, 33, 2), dtype=torch.int32), torch.zeros((1, 33), dtype=torch.int32), torch.zeros((1, 33)))
    for bad, kw in (([], {}), ([wide, wide], {}), ([a, b], dict(model_weights=[1.0])), ([a, b], dict(model_weights=[1.0, 0.0])),
                    ([a, b], dict(model_weights=[1.0, np.nan])), ([a, (b[0].long(), b[1], b[2])], {}), ([a, (b[0], b[1], b[2].double())], {}),
                    ([a, (b[0], b[1][:, :0], b[2])], {}), ([a, (b[0].repeat(2, 1, 1), b[1].repeat(2, 1), b[2].repeat(2, 1))], {}), ([a[:2]], {})):
        with pytest.raises(ValueError):
            mbr.pool_nbest(bad, **kw)


def test_host_side_refusals():
    for N, T, Cc, mode in ((0, 5, 60, 0), (65, 5, 60, 0), (4, 0, 60, 0), (4, 4097, 60, 0), (4, 5, 1, 0), (4, 5, 65, 0), (4, 5, 60, 2), (4, 5, 60, "x")):
        with pytest.raises(ValueError):
            mbr.check_device_args(N, T, Cc, mode)
    assert mbr.check_device_args(64, 4096, 64, "normalised") == 1 and mbr.check_device_args(1, 1, 2, 0) == 0
    for t in (0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            mbr.inverse_temperature(t)
    assert mbr.inverse_temperature(4) == 0.25
    with pytest.raises(ValueError):
        mbr.mbr_reference([], scores=[])
    with pytest.raises(ValueError):
        mbr.mbr_reference([[1]])
    with pytest.raises(ValueError):
        mbr.mbr_reference([[1]], scores=[0], mode=3)
    with pytest.raises(ValueError):
        mbr.mbr_reference([[1]], votes=[1, 2])
    idx, ln, sc = torch.zeros((1, 2, 3), dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 2))
    with pytest.raises(ValueError, match="GPU"):
        mbr.mbr_select(idx, ln, sc)                       # the kernel has no CPU path
    with pytest.raises(ValueError):
        mbr.mbr_select(idx.numpy(), ln, sc)
    # the wrappers' option
    class Stub:
        C, T, device = 60, 176, None
    class Beam:
        width = 4
    assert _mbr_setup(Stub, 4, None, 0, 1.0, True) is None          # off: nothing is looked at, nothing allocated
    for beam, nbest in ((Beam, 1), (Beam, -2), (None, 2), (Beam, 5)):
        with pytest.raises(ValueError):
            _mbr_setup(Stub, 4, beam, nbest, 1.0, True)
    with pytest.raises(ValueError):
        _set_mbr_temperature(None, 1.0)
    with pytest.raises(ValueError, match="mbr_nbest"):
        StreamingTFLiteModel(None, mbr_nbest=4)


def test_entry_point_refuses_before_any_hip_call(lib):
    """bad limits, null and misaligned buffers are refused with a message; B = 0 is a no-op.  None of these reaches the device: this runs
    without a GPU."""
    buf = (C.c_int32 * 64)()
    p = C.addressof(buf)
    ok = dict(hyp_idx=p, hyp_len=p + 64, hyp_score=p + 128, weights=None, inv_temp=None, B=1, N=2, T=3, C=60, mode=0, out_idx=p + 192, out_len=p + 224,
              best=p + 228, risk=None, w_out=None, dist=None, status=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ishara_mbr_select(a["hyp_idx"], a["hyp_len"], a["hyp_score"], a["weights"], a["inv_temp"], a["B"], a["N"], a["T"], a["C"], a["mode"],
                                     a["out_idx"], a["out_len"], a["best"], a["risk"], a["w_out"], a["dist"], a["status"], None)
    assert call(B=0) == 0
    for kw in (dict(N=0), dict(N=65), dict(T=0), dict(T=4097), dict(C=1), dict(C=65), dict(mode=2), dict(mode=-1), dict(B=-1), dict(hyp_idx=None),
               dict(hyp_len=None), dict(hyp_score=None), dict(out_idx=None), dict(out_len=None), dict(best=None), dict(hyp_idx=p + 2), dict(status=p + 1),
               dict(inv_temp=p + 3), dict(out_idx=p + 8)):
        assert call(**kw) == -1, kw
        assert b"ishara_mbr_select" in lib.ishara_last_error(), kw
