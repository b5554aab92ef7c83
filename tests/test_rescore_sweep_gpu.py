"""GPU: ishara_rescore_sweep (csrc/rescore_sweep.hip) and ishara_nbest_rescore_p (csrc/nbest_rescore.hip) over the cases of
tests/rescore_sweep_parity.py and tests/rescore_parity.py.
  sweep        best, dist, tlen and hyp_dist equal rescore_sweep_reference integer for integer with either fallback, lm_score equals the
               float32 walk bit for bit; the outputs start poisoned, sit between guard words at addresses that are 4-byte aligned and no
               more, and the guards survive
  composition  G x (ishara_nbest_rescore_p + ishara_edit_distance) on the device gives the same integers
  part A       the _p entry and the by-value entry write identical bytes; a captured _p launch follows rewritten params
  the rest     determinism, a captured sweep follows a rewritten grid, B = 0, the refusals"""
import ctypes

import numpy as np
import pytest
import torch

import rescore_parity as RP
import rescore_sweep_parity as SP
from ishara_amd import _lib, mbr, rescore

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in SP.cases()}
GUARD = 0x5A5A5A5


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _odd(n, dtype):
    """n elements of device memory at an address that is 4-byte aligned and not 8-byte aligned"""
    t = torch.empty(n + 3, dtype=dtype, device="cuda")
    t = t[1:] if t.data_ptr() % 8 == 0 else t
    assert t.data_ptr() % 8 == 4
    return t[:n]


class Arena:
    """best | dist | tlen | hyp_dist | lm_score in one int32 buffer, a guard word in front of, between and behind them, every output poisoned"""

    def __init__(self, G, B, N):
        sizes = dict(best=G * B, dist=G * B, tlen=B, hyp_dist=B * N, lm_score=B * N)
        self.buf = _odd(sum(sizes.values()) + len(sizes) + 1, torch.int32)
        self.buf.fill_(GUARD)
        self.guards, self.t, o = [0], {}, 1
        for k, n in sizes.items():
            self.t[k] = self.buf[o:o + n]
            if k == "lm_score":
                self.t[k] = self.t[k].view(torch.float32)
                self.t[k].fill_(float("nan"))
            else:
                self.t[k].fill_(-77)
            o += n
            self.guards.append(o)
            o += 1
        self.shape = dict(best=(G, B), dist=(G, B), tlen=(B,), hyp_dist=(B, N), lm_score=(B, N))

    def read(self):
        torch.cuda.synchronize()
        assert (self.buf[self.guards].cpu().numpy() == GUARD).all(), "a guard word was overwritten"
        return {k: v.cpu().numpy().reshape(self.shape[k]) for k, v in self.t.items()}


def _inputs(case):
    grid = _odd(case["grid"].size, torch.float32)
    grid.copy_(torch.from_numpy(np.array(case["grid"]).ravel()))
    return dict(idx=_dev(case["hyp_idx"]), ln=_dev(case["hyp_len"]), logps=[_dev(case["logps"][m]) for m in range(case["M"])], tgt=_dev(case["targets"]),
                grid=grid, lm=rescore.lm_to_device(case["lm"], "cuda", case["blank"]))


def _sweep(lib, case, d, fallback, out, optional=True):
    rescore.sweep_launch(lib, d["idx"], d["ln"], case["B"], case["N"], case["Th"], rescore.pointer_array(d["logps"]), case["M"], d["lm"], case["blank"],
                         d["tgt"], case["L"], fallback, d["grid"], case["G"], out.t["best"], out.t["dist"], out.t["tlen"],
                         out.t["hyp_dist"] if optional else None, out.t["lm_score"] if optional else None, None, _lib.stream())


# ------------------------------------------------------------------------------------------------ 1. every case against the reference
@pytest.mark.parametrize("fallback", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_sweep_equals_the_reference(lib, name, fallback):
    case = CASES[name]
    d = _inputs(case)
    out = Arena(case["G"], case["B"], case["N"])
    _sweep(lib, case, d, fallback, out)
    got = out.read()
    assert not SP.compare(case, fallback, got), SP.compare(case, fallback, got)
    assert np.array_equal(_bits(got["lm_score"]), _bits(SP.lm_walk(case))), "lm_score is not the float32 walk"
    bare = Arena(case["G"], case["B"], case["N"])            # the optional outputs as NULL: the rest the same, the two untouched
    _sweep(lib, case, d, fallback, bare, optional=False)
    b = bare.read()
    assert all(np.array_equal(b[k], got[k]) for k in ("best", "dist", "tlen")) and (b["hyp_dist"] == -77).all() and np.isnan(b["lm_score"]).all()
    if fallback == 1:                                        # the public wrapper gives the same tensors
        pub = rescore.rescore_sweep(d["idx"], d["ln"], d["logps"], d["tgt"], np.array(case["grid"]), case["lm"], case["blank"], True, return_details=True)
        assert all(np.array_equal(t.cpu().numpy(), got[k]) for t, k in zip(pub[:3], ("best", "dist", "tlen")))
        assert np.array_equal(pub[3]["hyp_dist"].cpu().numpy(), got["hyp_dist"]) and np.array_equal(_bits(pub[3]["lm_score"].cpu().numpy()), _bits(got["lm_score"]))


def test_sweep_on_the_devices_own_scores_with_rows_wider_than_the_model(lib):
    """Th != T: the scores come from ishara_ctc_score_nbest under logits of T = 96 frames, the hypothesis rows are 80 wide"""
    case = CASES["lengths"]
    assert case["Th"] == 80 and case["M"] == 1
    g = np.random.default_rng(77)
    x = _dev((g.standard_normal((case["B"], 96, 60)) * 2).astype(np.float32))
    d = _inputs(case)
    logp = rescore.ctc_score_nbest(x, d["idx"], d["ln"])
    d["logps"] = [logp]
    lp = logp.cpu().numpy()[None]
    assert np.isfinite(lp[0][np.asarray(case["hyp_len"]) >= 0]).all()
    lists = mbr.nbest_to_lists(case["hyp_idx"], case["hyp_len"])
    for fallback in (0, 1):
        out = Arena(case["G"], case["B"], case["N"])
        _sweep(lib, case, d, fallback, out)
        got = out.read()
        for clip in range(case["B"]):
            best, dist, tlen, hd = rescore.rescore_sweep_reference(lists[clip], lp[:, clip], case["targets"][clip], case["grid"], None, case["blank"], bool(fallback))
            assert np.array_equal(got["best"][:, clip], best) and np.array_equal(got["dist"][:, clip], dist) and got["tlen"][clip] == tlen
            assert np.array_equal(got["hyp_dist"][clip], hd)


# ------------------------------------------------------------------------------------------------ 2. the loop it replaces, on the device
@pytest.mark.parametrize("name", ["duplicates-none", "duplicates-bigram", "duplicates-ngram4"])
def test_sweep_equals_the_device_composition(lib, name):
    case = CASES[name]
    assert case["G"] == 7
    B, N, Th, M, G = case["B"], case["N"], case["Th"], case["M"], case["G"]
    d = _inputs(case)
    out = Arena(G, B, N)
    _sweep(lib, case, d, 1, out)
    got = out.read()
    oi, ol = torch.empty((B, N, Th), dtype=torch.int32, device="cuda"), torch.empty((B, N), dtype=torch.int32, device="cuda")
    osc, perm = torch.empty((B, N), device="cuda"), torch.empty((B, N), dtype=torch.int32, device="cuda")
    dist, tlen = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    grid = d["grid"].view(G, M + 2)
    for g in range(G):
        params = grid[g].clone()
        rescore.launch_p(lib, d["idx"], d["ln"], B, N, Th, rescore.pointer_array(d["logps"]), M, params, d["lm"], case["blank"], None, oi, ol, osc, None, perm,
                         _lib.stream())
        top_idx, top_len = oi[:, 0].contiguous(), ol[:, 0].contiguous()
        _lib.check(lib.ishara_edit_distance(_lib.ptr(top_idx), _lib.ptr(top_len), B, Th, _lib.ptr(d["tgt"]), case["L"], _lib.ptr(dist), _lib.ptr(tlen),
                                            _lib.stream()), "ishara_edit_distance")
        want_best = np.where(top_len.cpu().numpy() < 0, -1, perm[:, 0].cpu().numpy())
        assert np.array_equal(got["best"][g], want_best) and np.array_equal(got["dist"][g], dist.cpu().numpy()), (name, g)
        assert np.array_equal(got["tlen"], tlen.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 3. part A
RESCORE = {c["name"]: c for c in RP.rescore_cases()}


def _rescore_both(lib, case, params_d=None):
    """(by-value outputs, _p outputs) of one rescore_parity case fed the host's float32 scores"""
    B, N, Th, M = case["B"], case["N"], case["Th"], case["M"]
    lp = RP.host_logps(case)
    idx, ln, logps = _dev(case["hyp_idx"]), _dev(case["hyp_len"]), [_dev(lp[m]) for m in range(M)]
    w_d = _dev(case["weights"])
    it_d = None if case["inv_temp"] is None else _dev(np.array([case["inv_temp"]], np.float32))
    lm_dev = rescore.lm_to_device(case["lm"], "cuda", case["blank"])
    if params_d is None:
        params_d = _odd(M + 2, torch.float32)
        params_d.copy_(torch.from_numpy(np.concatenate([case["weights"], np.float32([case["alpha"], case["beta"]])])))

    def bufs():
        return dict(out_idx=_dev(np.full((B, N, Th), -77, np.int32)), out_len=_dev(np.full((B, N), -77, np.int32)), out_score=_dev(np.full((B, N), np.nan, np.float32)),
                    posterior=_dev(np.full((B, N), np.nan, np.float32)), perm=_dev(np.full((B, N), -77, np.int32)))

    a, p = bufs(), bufs()
    rescore.launch(lib, idx, ln, B, N, Th, rescore.pointer_array(logps), M, w_d, lm_dev, case["blank"], case["alpha"], case["beta"], it_d, a["out_idx"], a["out_len"],
                   a["out_score"], a["posterior"], a["perm"], _lib.stream())
    run_p = lambda: rescore.launch_p(lib, idx, ln, B, N, Th, rescore.pointer_array(logps), M, params_d, lm_dev, case["blank"], it_d, p["out_idx"],      # noqa: E731
                                     p["out_len"], p["out_score"], p["posterior"], p["perm"], _lib.stream())
    run_p()
    return a, p, run_p, params_d, lp, (idx, ln, logps)


@pytest.mark.parametrize("name", sorted(RESCORE))
def test_the_p_entry_writes_the_by_value_entrys_bytes(lib, name):
    case = RESCORE[name]
    a, p, _, params_d, lp, (idx, ln, logps) = _rescore_both(lib, case)
    torch.cuda.synchronize()
    for k in a:
        assert np.array_equal(a[k].cpu().numpy().view(np.uint32), p[k].cpu().numpy().view(np.uint32)), k
    assert not RP.check_rescore(case, {k: v.cpu().numpy() for k, v in p.items()}, lp)[0]
    pub = rescore.rescore_nbest(idx, ln, logps, lm=case["lm"], temperature=1.0 if case["inv_temp"] is None else _dev(np.array([case["inv_temp"]], np.float32)),
                                return_details=True, blank=case["blank"], params=params_d.clone())
    assert torch.equal(pub[0], a["out_idx"]) and torch.equal(pub[3]["perm"], a["perm"])
    assert np.array_equal(_bits(pub[2].cpu().numpy()), _bits(a["out_score"].cpu().numpy()))


def test_a_captured_p_launch_follows_rewritten_params(lib):
    case = RESCORE["bigram"]
    params_d = torch.zeros(case["M"] + 2, device="cuda")
    params_d.copy_(torch.from_numpy(np.concatenate([case["weights"], np.float32([case["alpha"], case["beta"]])])))
    a, p, run_p, _, lp, _ = _rescore_both(lib, case, params_d)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_p()
    new = np.float32([0.25, 0.0, 1.5, -0.6])
    params_d.copy_(torch.from_numpy(new))
    graph.replay()
    torch.cuda.synchronize()
    changed = dict(case, weights=new[:2], alpha=float(new[2]), beta=float(new[3]))
    got = {k: v.cpu().numpy() for k, v in p.items()}
    assert not RP.check_rescore(changed, got, lp)[0]
    assert not np.array_equal(_bits(got["out_score"]), _bits(a["out_score"].cpu().numpy()))
    # a non-finite beta is not refused by this entry: the arithmetic is IEEE's (inf * 0 is NaN) and the order is the contract's
    params_d.copy_(torch.from_numpy(np.float32([1, 1, 0.5, np.inf])))
    graph.replay()
    torch.cuda.synchronize()
    lists = mbr.nbest_to_lists(case["hyp_idx"], case["hyp_len"])
    for b in range(case["B"]):
        order = rescore.rescore_reference(lists[b], lp[:, b], np.float32([1, 1]), case["lm"], 0.5, float("inf"), 1.0, case["blank"])[0]
        assert np.array_equal(p["perm"][b].cpu().numpy(), order)


# ------------------------------------------------------------------------------------------------ 4. determinism, capture, empty batch, refusals
def test_two_sweeps_are_bit_identical_and_a_captured_sweep_follows_a_rewritten_grid(lib):
    case = CASES["r-N64-M3-G65-bigram"]
    d = _inputs(case)
    a, b = Arena(case["G"], case["B"], case["N"]), Arena(case["G"], case["B"], case["N"])
    _sweep(lib, case, d, 1, a)
    _sweep(lib, case, d, 1, b)
    ga, gb = a.read(), b.read()
    assert all(np.array_equal(ga[k].view(np.uint32) if ga[k].dtype == np.float32 else ga[k], gb[k].view(np.uint32) if gb[k].dtype == np.float32 else gb[k]) for k in ga)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _sweep(lib, case, d, 1, b)
    other = SP.random_grid(np.random.default_rng(99), case["G"], case["M"])
    d["grid"].copy_(torch.from_numpy(other.ravel()))
    graph.replay()
    got = b.read()
    lists = mbr.nbest_to_lists(case["hyp_idx"], case["hyp_len"])
    for clip in range(case["B"]):
        best, dist, _, _ = rescore.rescore_sweep_reference(lists[clip], case["logps"][:, clip], case["targets"][clip], other, case["lm"], case["blank"], True)
        assert np.array_equal(got["best"][:, clip], best) and np.array_equal(got["dist"][:, clip], dist), clip
    assert not np.array_equal(got["best"], ga["best"])


def test_an_empty_batch_is_a_no_op_and_the_workspace_is_answered(lib):
    case = CASES["C3"]
    d = _inputs(case)
    out = Arena(case["G"], case["B"], case["N"])
    rescore.sweep_launch(lib, d["idx"], d["ln"], 0, case["N"], case["Th"], rescore.pointer_array(d["logps"]), case["M"], d["lm"], case["blank"], d["tgt"], case["L"],
                         1, d["grid"], case["G"], out.t["best"], out.t["dist"], out.t["tlen"], out.t["hyp_dist"], out.t["lm_score"], None, _lib.stream())
    got = out.read()
    assert all((got[k] == -77).all() for k in ("best", "dist", "tlen", "hyp_dist")) and np.isnan(got["lm_score"]).all()
    assert lib.ishara_rescore_sweep_workspace_bytes(3, 5, 7) >= 0 and lib.ishara_rescore_sweep_workspace_bytes(0, 64, 65536) >= 0
    assert lib.ishara_rescore_sweep_workspace_bytes(3, 65, 7) < 0 and lib.ishara_rescore_sweep_workspace_bytes(3, 5, 0) < 0
    assert lib.ishara_rescore_sweep_workspace_bytes(3, 5, 65537) < 0 and lib.ishara_rescore_sweep_workspace_bytes(-1, 5, 7) < 0


def test_refusals_return_the_message_and_launch_nothing(lib):
    case = CASES["duplicates-bigram"]
    d = _inputs(case)
    out = Arena(case["G"], case["B"], case["N"])
    base = dict(hyp_idx=d["idx"], hyp_len=d["ln"], B=case["B"], N=case["N"], Th=case["Th"], logps=d["logps"], M=case["M"], lm_logp=d["lm"].logp, lm_next=d["lm"].next,
                S=d["lm"].S, start=d["lm"].start, C=60, blank=59, targets=d["tgt"], L=case["L"], fallback=1, grid=d["grid"], G=case["G"], best=out.t["best"],
                dist=out.t["dist"], tlen=out.t["tlen"], hyp_dist=out.t["hyp_dist"], lm_score=out.t["lm_score"])

    def call(**kw):
        a = dict(base, **kw)
        p = lambda t: t if isinstance(t, ctypes.c_void_p) else _lib.ptr(t)      # noqa: E731
        ptrs = rescore.pointer_array(a["logps"]) if a["logps"] is not None else None
        rc = lib.ishara_rescore_sweep(p(a["hyp_idx"]), p(a["hyp_len"]), a["B"], a["N"], a["Th"], ptrs, a["M"], p(a["lm_logp"]), p(a["lm_next"]), a["S"], a["start"],
                                      a["C"], a["blank"], p(a["targets"]), a["L"], a["fallback"], p(a["grid"]), a["G"], p(a["best"]), p(a["dist"]), p(a["tlen"]),
                                      p(a["hyp_dist"]), p(a["lm_score"]), None, _lib.stream())
        return rc, lib.ishara_last_error().decode()

    odd = ctypes.c_void_p(out.t["best"].data_ptr() + 2)
    bad = [(dict(N=0), "N=0"), (dict(N=65), "N=65"), (dict(Th=0), "Th=0"), (dict(Th=4097), "Th=4097"), (dict(M=0), "M=0"), (dict(M=9), "M=9"), (dict(B=-1), "B=-1"),
           (dict(G=0), "G=0"), (dict(G=65537), "G=65537"), (dict(L=0), "L=0"), (dict(L=65), "L=65"), (dict(fallback=2), "fallback"), (dict(fallback=-1), "fallback"),
           (dict(C=1), "C=1"), (dict(C=65), "C=65"), (dict(blank=60), "blank"), (dict(S=0), "S=0"), (dict(start=d["lm"].S), "start_state"),
           (dict(lm_next=None), "go together"), (dict(hyp_idx=None), "null hyp_idx"), (dict(logps=None), "null logp"), (dict(targets=None), "null targets"),
           (dict(grid=None), "null targets / grid"), (dict(best=None), "null best"), (dict(dist=None), "null best"), (dict(tlen=None), "null best"),
           (dict(best=odd), "misaligned"), (dict(best=d["tgt"]), "best overlaps targets"), (dict(dist=d["grid"]), "dist overlaps grid"),
           (dict(hyp_dist=d["ln"]), "hyp_dist overlaps hyp_len"), (dict(lm_score=d["logps"][1]), "lm_score overlaps logp[1]"), (dict(tlen=d["idx"]), "tlen overlaps hyp_idx")]
    for kw, word in bad:
        rc, msg = call(**kw)
        assert rc == -1 and "ishara_rescore_sweep" in msg and word in msg, (kw.keys(), rc, msg)
    got = out.read()
    assert all((got[k] == -77).all() for k in ("best", "dist", "tlen", "hyp_dist")) and np.isnan(got["lm_score"]).all(), "a refused call wrote something"
    rc, _ = call()
    assert rc == 0
    assert not SP.compare(case, 1, out.read())
    # the _p entry refuses what its sibling refuses, and a null params
    c = RESCORE["M1"]
    z = torch.zeros((c["B"], c["N"], c["Th"]), dtype=torch.int32, device="cuda")
    rc = lib.ishara_nbest_rescore_p(_lib.ptr(z), _lib.ptr(z), c["B"], c["N"], c["Th"], rescore.pointer_array([z]), 1, None, None, None, 0, 0, 0, 0, None, _lib.ptr(z),
                                    _lib.ptr(z), _lib.ptr(z), None, None, _lib.stream())
    assert rc == -1 and "ishara_nbest_rescore_p: null params" in lib.ishara_last_error().decode()
