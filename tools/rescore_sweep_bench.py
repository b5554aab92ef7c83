#!/usr/bin/env python3
"""What the rescoring weight sweep costs on the device (ishara_rescore_sweep) beside the loop it replaces.  Records, not pass marks:

  * at B 64, T 384 (the width of the hypothesis rows), C 60, hypotheses of 20 to 30 symbols, targets of 20 to 30 symbols, N = 8, 16, 32, 64,
    M = 1 and 4 models, G = 64 and 1024 grid rows, without an LM and with the 5-gram automaton of tools/nbest_rescore_bench.py: HIP-event
    time around one ishara_rescore_sweep call (device idle before each; median, min, max, 10th and 90th percentile) against the loop
    G x (ishara_nbest_rescore_p on grid[g] + ishara_edit_distance), the two legs alternated in rounds in one process.  The loop's edit
    distance runs over all B * N rows of the rescored list in one launch (row b * N is the top row), so the loop holds no copy and no
    torch operation; its 2 G launches are issued from Python, and where the host issues them more slowly than the device runs them the
    event pair measures the host.  Both legs are checked for equal integers in the same run;
  * three replay times of BatchedTFLiteModel (configs[1]-sized bf16 model, batch 64, beam width 16): with rescore_nbest = 8, without
    it, and (--parent: a JSON written by --plain-only from a checkout of the parent commit in the same visit) the plain replay there.
No accuracy figure: there is no dataset and there are no trained weights.

    python tools/rescore_sweep_bench.py --out profiles/r24_rescore_sweep.json [--parent parent_plain.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, CN, L = 64, 384, 60, 32
NS, MS, GS = (8, 16, 32, 64), (1, 4), (64, 1024)
ROUNDS = 3
MODEL_KW = dict(dim=256, num_conv_squeeze_blocks=2, num_conv_conform_blocks=2, kernel_sizes=[11, 5, 3], num_conv_per_block=3,
                dropout_rate=0.2, num_heads=8, expansion_factor=2, transformer_kernel_size=15, input_shape=(T, 276))


def spread(ts):
    ts = np.sort(np.asarray(ts, np.float64))
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts[0]), max_ms=float(ts[-1]), p10_ms=float(np.percentile(ts, 10)),
                p90_ms=float(np.percentile(ts, 90)), reps=int(ts.size))


def event_ms(fn, reps, warmup=2):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def nbest(g, N):
    """per clip a target of 20 to 30 symbols and N hypotheses: copies of it with three symbols changed, cut to 20 to 30 symbols"""
    idx = np.full((B, N, T), -1, np.int32)
    ln = g.integers(20, 31, (B, N)).astype(np.int32)
    tgt = np.full((B, L), 59, np.int32)
    for b in range(B):
        base = g.integers(0, CN - 1, 32)
        tl = int(g.integers(20, 31))
        tgt[b, :tl] = base[:tl]
        for n in range(N):
            h = base.copy()
            h[g.integers(0, 32, 3)] = g.integers(0, CN - 1, 3)
            idx[b, n, :ln[b, n]] = h[:ln[b, n]]
    return idx, ln, tgt


def sweeps():
    import torch
    from ishara_amd import _lib, rescore
    from ishara_amd.ctc_lm import CharNGramLM
    lib = _lib.load()
    g = np.random.default_rng(1)
    lm = CharNGramLM.fit([g.integers(0, CN - 1, int(g.integers(5, 31))).tolist() for _ in range(2000)], order=5, num_classes=CN)
    lm_dev = rescore.lm_to_device(lm, "cuda")
    rows = []
    for N in NS:
        idx, ln, tgt = nbest(g, N)
        d_idx, d_ln, d_tgt = torch.from_numpy(idx).cuda(), torch.from_numpy(ln).cuda(), torch.from_numpy(tgt).cuda()
        d_tgt_all = d_tgt.repeat_interleave(N, dim=0).contiguous()                    # the loop's edit distance takes every row of the list
        o_idx, o_len = torch.empty((B, N, T), dtype=torch.int32, device="cuda"), torch.empty((B, N), dtype=torch.int32, device="cuda")
        o_sc, o_perm = torch.empty((B, N), device="cuda"), torch.empty((B, N), dtype=torch.int32, device="cuda")
        d_all, t_all = torch.empty(B * N, dtype=torch.int32, device="cuda"), torch.empty(B * N, dtype=torch.int32, device="cuda")
        for M in MS:
            logps = [torch.from_numpy((-60 - 20 * g.random((B, N))).astype(np.float32)).cuda() for _ in range(M)]
            ptrs = rescore.pointer_array(logps)
            for G in GS:
                grid = np.concatenate([g.uniform(0, 2, (G, M)), g.uniform(0, 1, (G, 1)), g.uniform(-2, 2, (G, 1))], axis=1).astype(np.float32)
                d_grid = torch.from_numpy(grid).cuda()
                best, dist = torch.empty((G, B), dtype=torch.int32, device="cuda"), torch.empty((G, B), dtype=torch.int32, device="cuda")
                tlen = torch.empty(B, dtype=torch.int32, device="cuda")
                for name, dev in (("none", None), ("5-gram", lm_dev)):
                    st = _lib.stream()

                    def sweep():
                        rescore.sweep_launch(lib, d_idx, d_ln, B, N, T, ptrs, M, dev, CN - 1, d_tgt, L, 1, d_grid, G, best, dist, tlen, None, None, None, st)

                    def row(gi):
                        rescore.launch_p(lib, d_idx, d_ln, B, N, T, ptrs, M, d_grid[gi], dev, CN - 1, None, o_idx, o_len, o_sc, None, o_perm, st)
                        _lib.check(lib.ishara_edit_distance(_lib.ptr(o_idx), _lib.ptr(o_len), B * N, T, _lib.ptr(d_tgt_all), L, _lib.ptr(d_all), _lib.ptr(t_all), st),
                                   "ishara_edit_distance")

                    def loop():
                        for gi in range(G):
                            row(gi)

                    t = dict(sweep=[], loop=[])
                    for _ in range(ROUNDS):                  # alternated: the legs share whatever else the host is doing
                        t["sweep"] += event_ms(sweep, reps=10)
                        t["loop"] += event_ms(loop, reps=3 if G > 64 else 6, warmup=1)
                    sweep()
                    same = True
                    for gi in range(G):                      # the loop's integers, row by row, against the sweep's
                        row(gi)
                        want_best = torch.where(o_len[:, 0] < 0, torch.full_like(o_perm[:, 0], -1), o_perm[:, 0])
                        same = same and bool(torch.equal(best[gi], want_best)) and bool(torch.equal(dist[gi], d_all.view(B, N)[:, 0]))
                    r = dict(N=N, M=M, G=G, lm=name, lm_states=lm_dev.S if dev is not None else 0, integers_equal=same, sweep=spread(t["sweep"]), loop=spread(t["loop"]))
                    r["faster_by_more_than_the_spreads"] = bool(r["sweep"]["p90_ms"] < r["loop"]["p10_ms"])
                    r["loop_over_sweep_at_median"] = r["loop"]["median_ms"] / r["sweep"]["median_ms"]
                    rows.append(r)
    return rows


def replays(plain_only):
    import torch
    from ishara_amd import get_model
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    g = np.random.default_rng(0)
    clips = [g.standard_normal((int(n), 276)).astype(np.float32) for n in g.integers(25, 700, B)]
    model = get_model(**MODEL_KW, dtype="bf16", max_batch=B, seed=0)
    plain = BatchedTFLiteModel(model, batch_size=B, max_frames=1024, beam_width=16)
    plain.predict_indices(clips)                          # captures the graph and leaves the batch resident in device slot 0
    second = None
    if not plain_only:
        second = BatchedTFLiteModel(model, batch_size=B, max_frames=1024, beam_width=16, rescore_nbest=8, rescore_beta=0.5)
        second.predict_indices(clips)
    t_plain, t_second = [], []
    for _ in range(4):                                    # alternated: 4 rounds of 25 replays each way
        t_plain += event_ms(lambda: plain._run(0, False), reps=25, warmup=2)
        if second is not None:
            t_second += event_ms(lambda: second._run(0, False), reps=25, warmup=2)
    res = dict(batch=B, beam_width=16, beam_top1_replay=spread(t_plain))
    if second is not None:
        res.update(rescore_nbest=8, rescore_replay=spread(t_second), added_ms_at_median=spread(t_second)["median_ms"] - spread(t_plain)["median_ms"])
    torch.cuda.synchronize()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain-only", action="store_true", help="only the beam wrapper's replay (runs on a checkout without the sweep)")
    ap.add_argument("--parent", default=None, help="the JSON a --plain-only run on the parent commit wrote in the same visit")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("rescore_sweep_bench: no GPU: nothing here can be measured on the host")
    from ishara_amd.build import source_hash
    if a.plain_only:
        res = dict(source_hash=source_hash(), device=torch.cuda.get_device_name(0), replays=replays(True))
    else:
        res = dict(workload=f"ishara_rescore_sweep beside G x (ishara_nbest_rescore_p + ishara_edit_distance) at B {B}, C {CN}, hypotheses and targets of "
                            f"20..30 symbols in rows of width {T}",
                   source_hash=source_hash(), device=torch.cuda.get_device_name(0), sweep=sweeps(), replays=replays(False),
                   note="event pairs around single calls with the device idle before each, the two legs alternated in rounds in one process; the loop's "
                        "2 G launches are issued from Python.  No accuracy effect is measured: there is no dataset and there are no trained weights")
        if a.parent:
            with open(a.parent) as f:
                p = json.load(f)
            res["replays"]["parent_commit"] = dict(source_hash=p["source_hash"], beam_top1_replay=p["replays"]["beam_top1_replay"])
            mine, theirs = res["replays"]["beam_top1_replay"], p["replays"]["beam_top1_replay"]
            res["replays"]["off_path_unmoved_within_its_spread"] = bool(mine["p10_ms"] <= theirs["p90_ms"] and theirs["p10_ms"] <= mine["p90_ms"])
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
