#!/usr/bin/env python3
"""One-off comparison of this build with a library built from the parent commit's csrc, for the change that moved the CTC lattice
arithmetic into csrc/ctc_lattice.h and the bit-vector edit distance into csrc/edit_distance.h (profiles/r27_ctc_lattice.json).

  Bits.  Every entry point whose kernel the change touched runs from both libraries on the same seeded inputs, every output buffer
  pre-filled with the same bytes, and every output must be byte-equal: ishara_ctc_loss / _ex / ishara_op_ctc_loss (nll, dlogits, dlb),
  ishara_ctc_score_nbest (logp, status), ishara_ctc_nbest_grad with accumulate 0 and 1 (dlogits, dlb, logp, status), ishara_kd_grad,
  ishara_mbr_select, ishara_rescore_sweep, ishara_mwer_weights, ishara_edit_distance, ishara_edit_alignment.  The inputs are the tests'
  case tables (every case family of ctc_parity, each also with seeded per-sample frame counts for _ex; ctc_lengths_parity's tails,
  seams, contract and scaled tables with their pad kinds, bad lengths, sample scales and zero_inf; rescore_parity.score_cases;
  mwer_parity.grad_cases / weight_cases; kd_parity; mbr_parity; rescore_sweep_parity WITHOUT its LM (NULL tables: its best / dist are
  compared under LM-free scores; the distance path does not read the LM); edit_alignment_parity) and the timed shapes.  The tolerance
  is zero: the change reorders no operation, the build has no fast-math, the distances are integers.
  Time.  This build, the parent and a second copy of the parent (A/A) alternate block by block: device events, a warm-up, the median over
  the blocks, every timed window a few milliseconds.  Accepted per point when new <= parent + |parent - parent_again|.

    python tools/ctc_lattice_compare.py --parent-lib PATH/libishara_hip.so --out profiles/r27_ctc_lattice.json

Needs a GPU: without one it fails, there is no fallback."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FILL = 0x5A                                                  # every output byte before a launch


def _foreign(path):
    from ishara_amd import _lib
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def _out(nbytes):
    import torch
    return torch.full((max(int(nbytes), 1),), FILL, dtype=torch.uint8, device="cuda")


def _values(table):
    return list(table.values()) if isinstance(table, dict) else list(table)


# ---------------------------------------------------------------------------------------------- the calls: name -> (run(lib), outputs)
def call_ctc(x, y, blank, entry, frame_len=None, gs=1.0, sample_scale=None, zero_inf=0):
    from ishara_amd import _lib
    p, st = _lib.ptr, _lib.stream
    B, T, Cn = x.shape
    L = y.shape[1]
    xd, yd, fl, ss = _dev(x), _dev(y), _dev(frame_len), _dev(sample_scale)
    outs = dict(nll=_out(4 * B), dlogits=_out(4 * B * T * Cn), dlb=_out(256 * B * T))

    def run(lib):
        ws = _out(lib.ishara_ctc_workspace_bytes(B, T, L))
        if entry == "ishara_ctc_loss":
            return lib.ishara_ctc_loss(p(xd), p(yd), B, T, Cn, L, blank, p(outs["nll"]), p(outs["dlogits"]), C.c_float(gs), p(ws), st())
        if entry == "ishara_op_ctc_loss":
            return lib.ishara_op_ctc_loss(p(xd), p(yd), B, T, Cn, L, blank, p(outs["nll"]), p(outs["dlogits"]), C.c_float(gs), p(ws), p(outs["dlb"]), st())
        return lib.ishara_ctc_loss_ex(p(xd), p(yd), B, T, Cn, L, blank, p(outs["nll"]), p(outs["dlogits"]), C.c_float(gs), p(ws), p(fl), p(ss), zero_inf, st())
    return run, outs


def call_score(c):
    from ishara_amd import _lib
    p, st = _lib.ptr, _lib.stream
    x, idx, ln, fl = _dev(c["logits"]), _dev(c["hyp_idx"]), _dev(c["hyp_len"]), _dev(c["frame_len"])
    outs = dict(logp=_out(4 * c["B"] * c["N"]), status=_out(4 * c["B"] * c["N"]))

    def run(lib):
        return lib.ishara_ctc_score_nbest(p(x), c["B"], c["T"], c["C"], c["blank"], p(idx), p(ln), c["N"], c["Th"], p(fl), p(outs["logp"]), p(outs["status"]), st())
    return run, outs


def call_nbest_grad(c, accumulate):
    from ishara_amd import _lib
    p, st = _lib.ptr, _lib.stream
    B, T, Cn, N = c["B"], c["T"], c["C"], c["N"]
    x, idx, ln, fl, cf = _dev(c["logits"]), _dev(c["hyp_idx"]), _dev(c["hyp_len"]), _dev(c["frame_len"]), _dev(c["coef"])
    outs = dict(dlogits=_out(4 * B * T * Cn), dlb=_out(256 * B * T), logp=_out(4 * B * N), status=_out(4 * B * N))
    if accumulate:                                           # the rows it adds to: finite numbers, the same for both libraries
        outs["dlogits"] = _dev(np.random.default_rng(5).standard_normal(B * T * Cn).astype(np.float32)).view(__import__("torch").uint8)

    def run(lib):
        ws = _out(lib.ishara_ctc_nbest_grad_workspace_bytes(B, T, N, c["max_len"]) + 16)
        wp = C.c_void_p((ws.data_ptr() + 15) // 16 * 16)
        return lib.ishara_ctc_nbest_grad(p(x), B, T, Cn, c["blank"], p(idx), p(ln), N, c["Th"], c["max_len"], p(fl), p(cf), C.c_float(c["grad_scale"]),
                                         p(outs["dlogits"]), accumulate, p(outs["dlb"]), p(outs["logp"]), p(outs["status"]), wp, st())
    return run, outs


def call_kd(c, accumulate):
    from ishara_amd import _lib
    p, st = _lib.ptr, _lib.stream
    B, T, Cn = c["B"], c["T"], c["C"]
    x, u, fl = _dev(c["logits"]), _dev(c["teacher"]), _dev(c["frame_len"])
    outs = dict(dlogits=_out(4 * B * T * Cn), dlb=_out(256 * B * T), kl_frame=_out(4 * B * T), kl_clip=_out(4 * B))
    if accumulate:
        outs["dlogits"] = _dev(np.random.default_rng(6).standard_normal(B * T * Cn).astype(np.float32)).view(__import__("torch").uint8)

    def run(lib):
        return lib.ishara_kd_grad(None, p(x), p(u), B, T, Cn, C.c_float(c["inv_temp"]), c["mode"], p(fl), C.c_float(c["grad_scale"]), p(outs["dlogits"]),
                                  accumulate, p(outs["dlb"]), p(outs["kl_frame"]), p(outs["kl_clip"]), st())
    return run, outs


def call_mbr(c):
    from ishara_amd import _lib
    p, st = _lib.ptr, _lib.stream
    B, N, T = c["B"], c["N"], c["T"]
    idx, ln, sc, w = _dev(c["hyp_idx"]), _dev(c["hyp_len"]), _dev(c["hyp_score"]), _dev(c["weights"])
    it = None if c["inv_temp"] is None else _dev(np.array([c["inv_temp"]], np.float32))
    outs = dict(out_idx=_out(4 * B * T), out_len=_out(4 * B), best=_out(4 * B), risk=_out(4 * B * N), w=_out(4 * B * N), dist=_out(4 * B * N * N), status=_out(4 * B))

    def run(lib):
        return lib.ishara_mbr_select(p(idx), p(ln), p(sc), p(w), p(it), B, N, T, c["C"], c["mode"], p(outs["out_idx"]), p(outs["out_len"]), p(outs["best"]),
                                     p(outs["risk"]), p(outs["w"]), p(outs["dist"]), p(outs["status"]), st())
    return run, outs


def call_sweep(c, fallback):
    from ishara_amd import _lib
    p, st = _lib.ptr, _lib.stream
    B, N, M, G = c["B"], c["N"], c["M"], c["G"]
    idx, ln, tg, grid = _dev(c["hyp_idx"]), _dev(c["hyp_len"]), _dev(c["targets"]), _dev(c["grid"])
    lps = [_dev(c["logps"][m]) for m in range(M)]
    ptrs = (C.c_void_p * M)(*[t.data_ptr() for t in lps])
    outs = dict(best=_out(4 * G * B), dist=_out(4 * G * B), tlen=_out(4 * B), hyp_dist=_out(4 * B * N), lm_score=_out(4 * B * N))

    def run(lib):
        return lib.ishara_rescore_sweep(p(idx), p(ln), B, N, c["Th"], ptrs, M, None, None, 0, 0, 0, 0, p(tg), c["L"], fallback, p(grid), G, p(outs["best"]),
                                        p(outs["dist"]), p(outs["tlen"]), p(outs["hyp_dist"]), p(outs["lm_score"]), None, st())
    return run, outs


def call_mwer_weights(c):
    from ishara_amd import _lib
    p, st = _lib.ptr, _lib.stream
    B, N = c["B"], c["N"]
    idx, ln, lp, stt, tg = _dev(c["hyp_idx"]), _dev(c["hyp_len"]), _dev(c["logp"]), _dev(c["status"]), _dev(c["targets"])
    it = None if c["inv_temp"] is None else _dev(np.array([c["inv_temp"]], np.float32))
    outs = dict(dist=_out(4 * B * N), post=_out(4 * B * N), risk=_out(4 * B), coef=_out(4 * B * N), tlen=_out(4 * B))

    def run(lib):
        return lib.ishara_mwer_weights(p(idx), p(ln), p(lp), p(stt), B, N, c["Th"], p(tg), c["L"], p(it), c["mode"], p(outs["dist"]), p(outs["post"]),
                                       p(outs["risk"]), p(outs["coef"]), p(outs["tlen"]), st())
    return run, outs


def call_edit(idx, ln, tg, fallback, align):
    from ishara_amd import _lib
    p, st = _lib.ptr, _lib.stream
    B, T = idx.shape
    L = tg.shape[1]
    di, dl, dt = _dev(idx), _dev(ln), _dev(tg)
    if not align:
        outs = dict(dist=_out(4 * B), tlen=_out(4 * B))
        return (lambda lib: lib.ishara_edit_distance(p(di), p(dl), B, T, p(dt), L, p(outs["dist"]), p(outs["tlen"]), st())), outs
    outs = dict(ops=_out(16 * B), aligned=_out(4 * B * L), inserted=_out(4 * B * (L + 1)), confusion=_out(4 * 60 * 60))

    def run(lib):
        ws = _out(lib.ishara_edit_alignment_workspace_bytes(B, T) + 16)
        wp = C.c_void_p((ws.data_ptr() + 15) // 16 * 16)
        return lib.ishara_edit_alignment(p(di), p(dl), B, T, p(dt), L, fallback, p(outs["ops"]), p(outs["aligned"]), p(outs["inserted"]), p(outs["confusion"]),
                                         wp, st())
    return run, outs


# ---------------------------------------------------------------------------------------------- the timed shapes (seeded)
def _hyps(g, B, N, Th, lo, hi, Cn=60):
    idx = np.full((B, N, Th), -1, np.int32)
    ln = g.integers(lo, hi + 1, (B, N)).astype(np.int32)
    for b in range(B):
        for n in range(N):
            idx[b, n, :ln[b, n]] = g.integers(0, Cn - 1, ln[b, n])
    return idx, ln


def timed_points():
    g = np.random.default_rng(27)
    pts = {}
    B, T, Cn, L = 256, 384, 60, 64
    x = (3.0 * g.standard_normal((B, T, Cn))).astype(np.float32)
    y = np.full((B, L), Cn - 1, np.int64)
    for i in range(B):
        n = int(g.integers(L // 8, L // 2 + 1))
        y[i, :n] = g.integers(0, Cn - 1, n)
    pts["ctc_loss B256 T384 L64 C60 dlogits"] = call_ctc(x, y, Cn - 1, "ishara_ctc_loss")
    xs = x[:64]
    for N in (16, 64):
        idx, ln = _hyps(g, 64, N, T, 20, 30)
        pts[f"ctc_score_nbest B64 T384 C60 N{N}"] = call_score(dict(logits=xs, hyp_idx=idx, hyp_len=ln, frame_len=None, B=64, T=T, C=Cn, blank=Cn - 1, N=N, Th=T))
    idx, ln = _hyps(g, 64, 8, T, 20, 30)
    coef = g.standard_normal((64, 8)).astype(np.float32)
    pts["ctc_nbest_grad B64 T384 N8 max_len32"] = call_nbest_grad(dict(logits=xs, hyp_idx=idx, hyp_len=ln, frame_len=None, coef=coef, B=64, T=T, C=Cn, blank=Cn - 1,
                                                                       N=8, Th=T, max_len=32, grad_scale=1.0), 0)
    idx, ln = _hyps(g, 256, 16, T, 20, 30)
    sc = g.standard_normal((256, 16)).astype(np.float32)
    pts["mbr_select B256 N16 T384"] = call_mbr(dict(hyp_idx=idx, hyp_len=ln, hyp_score=sc, weights=None, inv_temp=None, B=256, N=16, T=T, C=Cn, mode=0))
    idx, ln = _hyps(g, 256, 8, T, 0, 30)
    tg = np.full((256, 64), 59, np.int32)
    for b in range(256):
        n = int(g.integers(1, 33))
        tg[b, :n] = g.integers(0, 59, n)
    for G in (64, 1024):
        grid = np.abs(g.standard_normal((G, 3))).astype(np.float32)
        pts[f"rescore_sweep B256 N8 M1 G{G}"] = call_sweep(dict(hyp_idx=idx, hyp_len=ln, logps=sc[None, :, :8].copy() * np.ones((1, 256, 8), np.float32), targets=tg,
                                                                grid=grid, B=256, N=8, M=1, G=G, Th=T, L=64), 1)
    pts["mwer_weights B256 N8 Th384 L64"] = call_mwer_weights(dict(hyp_idx=idx, hyp_len=ln, logp=-np.abs(sc[:, :8]) - 3.0, status=None, targets=tg, inv_temp=None,
                                                                   mode=1, B=256, N=8, Th=T, L=64))
    return pts


def table_points():
    import ctc_lengths_parity as LP
    import ctc_parity as CP
    import edit_alignment_parity as EP
    import kd_parity as KP
    import mbr_parity as MP
    import mwer_parity as WP
    import rescore_parity as RP
    import rescore_sweep_parity as SP
    pts = {}
    fixed = [CP.case_a(L) for L in CP.A_LS] + [CP.case_b(L, T) for L in (8, 64) for T in CP.B_TS] + [CP.case_c(i) for i in range(len(CP.TIGHT))]
    fixed += [CP.case_d(i) for i in CP.D_IS] + [CP.case_e(Cc, bl) for Cc, bl in CP.E_CB]
    fixed += [CP.case_f(L, T, r) for L, T in CP.F_SHAPES for r in CP.REGIMES if r != "n2"] + [CP.case_g()]
    fixed += [CP.case_h(Cc, T, inf) for Cc in (60, 64, 33) for T in (9, 57) for inf in (False, True)] + [CP.case_j(B) for B in (1, 300)]
    fixed += [CP.case_k(Cc, v, pos) for Cc, v, pos in ((60, 60, 3), (60, 63, 0), (60, -1, 6), (33, 33, 3), (33, 63, 6), (33, -1, 0), (5, 5, 0), (5, 40, 3), (5, -1, 6))]
    for i, case in enumerate(fixed):                         # every family of tests/test_ctc_gpu.py
        x, y = np.asarray(CP.logits(case), np.float32), np.asarray(CP.labels(case), np.int64)
        fl = np.random.default_rng(i).integers(0, case.T + 2, case.B).astype(np.int32)      # 0 and T + 1: samples without frames
        pts[f"ctc_loss {case.name}"] = call_ctc(x, y, case.blank, "ishara_ctc_loss", gs=0.375)
        pts[f"op_ctc_loss {case.name}"] = call_ctc(x, y, case.blank, "ishara_op_ctc_loss")
        pts[f"ctc_loss_ex {case.name}"] = call_ctc(x, y, case.blank, "ishara_ctc_loss_ex", frame_len=fl)
    for rc, pads in ((LP.tails(), LP.PADS), (LP.seams(64), ("normal", "nan")), (LP.seams(255), ("normal", "nan")), (LP.contract(), LP.PADS),
                     (LP.scaled(), LP.PADS)):                # the tables of tests/test_ctc_lengths_gpu.py
        x, y, fl = LP.logits(rc), np.asarray(LP.labels(rc), np.int64), LP.frame_len(rc)
        for kind in pads:
            pts[f"ctc_loss_ex {rc.name} {kind}"] = call_ctc(LP.pad(x, fl, kind), y, rc.blank, "ishara_ctc_loss_ex", frame_len=fl)
    rc = LP.contract()
    fl = LP.frame_len(rc).astype(np.int64)
    fl[[1, 3, 5, 7]] = LP.BAD_LENGTHS
    pts["ctc_loss_ex contract bad lengths"] = call_ctc(np.asarray(LP.logits(rc), np.float32), np.asarray(LP.labels(rc), np.int64), rc.blank, "ishara_ctc_loss_ex",
                                                       frame_len=fl.astype(np.int32), gs=0.5)
    rc = LP.scaled()
    for zi in (0, 1):
        pts[f"ctc_loss_ex scaled zero_inf{zi}"] = call_ctc(LP.pad(LP.logits(rc), LP.frame_len(rc), "nan"), np.asarray(LP.labels(rc), np.int64), rc.blank,
                                                          "ishara_ctc_loss_ex", frame_len=LP.frame_len(rc), gs=0.5, sample_scale=LP.SCALES_ANY, zero_inf=zi)
    for c in _values(RP.score_cases()):
        pts[f"ctc_score_nbest {c['name']}"] = call_score(c)
    for c in _values(WP.grad_cases()):
        for acc in (0, 1):
            pts[f"ctc_nbest_grad acc{acc} {c['name']}"] = call_nbest_grad(c, acc)
    for c in _values(WP.weight_cases()):
        pts[f"mwer_weights {c['name']}"] = call_mwer_weights(c)
    for c in _values(KP.cases()):
        for acc in (0, 1):
            pts[f"kd_grad acc{acc} {c['name']}"] = call_kd(c, acc)
    for c in _values(MP.cases()):
        pts[f"mbr_select {c['name']}"] = call_mbr(c)
    for c in _values(SP.cases()):
        for fb in (0, 1):
            pts[f"rescore_sweep fb{fb} {c['name']}"] = call_sweep(c, fb)
    for T, L in EP.SHAPES:
        idx, ln, tg = EP.pack(EP.cases(T, L), T, L)[:3]
        idx, ln, tg = np.asarray(idx, np.int32), np.asarray(ln, np.int32), np.asarray(tg, np.int32)
        pts[f"edit_distance T{T} L{L}"] = call_edit(idx, ln, tg, 1, False)
        for fb in (0, 1):
            pts[f"edit_alignment fb{fb} T{T} L{L}"] = call_edit(idx, ln, tg, fb, True)
    return pts


# ---------------------------------------------------------------------------------------------- bits and time
def bits(points, new, parent):
    import torch
    bad, n, refused = [], 0, 0
    for name, (run, outs) in points.items():
        got, rcs = {}, {}
        for tag, lib in (("new", new), ("parent", parent)):
            saved = {k: v.clone() for k, v in outs.items()}
            rcs[tag] = run(lib)
            torch.cuda.synchronize()
            got[tag] = {k: v.clone() for k, v in outs.items()}
            for k, v in outs.items():
                v.copy_(saved[k])
        if rcs["new"] != rcs["parent"]:
            bad.append(f"{name}: return codes {rcs['new']} / {rcs['parent']}")
        refused += 1 if rcs["parent"] != 0 else 0           # refused by both alike: the untouched buffers are still compared
        for k in outs:
            n += 1
            if not torch.equal(got["new"][k], got["parent"][k]):
                bad.append(f"{name}: {k}")
    return dict(points=len(points), refused_by_both=refused, buffers=n, differing=bad, equal=not bad)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def timing(points, libs, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {}
    for name, (run, _) in points.items():
        def block_ms(lib, block):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(block):
                run(lib)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / block
        for lib in libs.values():
            block_ms(lib, 3)
        block = max(2, min(200, int(4.0 / max(block_ms(libs["parent"], 3), 1e-3))))      # a timed window of about 4 ms
        ts = {k: [] for k in libs}
        for _ in range(reps):
            for k, lib in libs.items():
                ts[k].append(block_ms(lib, block))
        ms = {k: _median(v) for k, v in ts.items()}
        aa = abs(ms["parent"] - ms["parent_again"])
        res[name] = dict(block=block, reps=reps, new_ms=ms["new"], parent_ms=ms["parent"], parent_again_ms=ms["parent_again"], aa_difference_ms=aa,
                         accepted=bool(ms["new"] <= ms["parent"] + aa))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libishara_hip.so built from the parent commit's csrc")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ctc_lattice_compare: no GPU (nothing is compared without one)")
    from ishara_amd import _lib
    from ishara_amd.build import source_hash
    tmp = tempfile.mkdtemp()
    copy = shutil.copy(a.parent_lib, os.path.join(tmp, "libishara_hip_parent_copy.so"))
    libs = dict(new=_lib.load(), parent=_foreign(os.path.abspath(a.parent_lib)), parent_again=_foreign(copy))
    timed = timed_points()
    res = dict(device=torch.cuda.get_device_name(0), source_hash=source_hash(),
               bits=bits({**table_points(), **timed}, libs["new"], libs["parent"]),
               timing_note="device events around a block of back-to-back launches, warmed up, median over the blocks; ms per launch",
               time=timing(timed, libs, a.reps))
    shutil.rmtree(tmp)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not res["bits"]["equal"]:
        raise SystemExit("ctc_lattice_compare: outputs differ from the parent's")
