#!/usr/bin/env python3
"""What second-pass n-best rescoring costs on the device (ishara_ctc_score_nbest, ishara_nbest_rescore).  Records, not pass marks:

  * the exact scores at B 64, T 384, C 60 for N = 8, 16, 32, 64 hypotheses of 20 to 30 symbols: HIP-event time around one
    ishara_ctc_score_nbest launch (device idle before each; median, min, max, 10th and 90th percentile), under the library's default
    slot-to-wave mapping and under 1, 2 and 4 slots per wave (ishara_debug_set_score_group);
  * beside it the emulation it replaces, which exists on the parent commit: ctc.ctc_loss(reduction="none") over the logits replicated N
    times, the replication and the workspace allocation included, alternated with the new kernel in one process; the bytes the emulation
    allocates (replicated logits + the two fp64 lattices) and whether its -nll has the new kernel's bits;
  * ishara_nbest_rescore at M = 1 and 4 models, without an LM and with a 5-gram automaton.
An event pair around a launch of a few microseconds includes the launch floor: such a figure is the cost of the call in a stream, not the
kernel's own time.  No accuracy figure: there is no dataset and there are no trained weights.

    python tools/nbest_rescore_bench.py --out profiles/r23_nbest_rescore.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, CN = 64, 384, 60
NS = (8, 16, 32, 64)
ROUNDS = 4


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
    """hypotheses of 20 to 30 symbols without the blank: per clip one base string, every slot a copy with three symbols changed"""
    idx = np.full((B, N, T), -1, np.int32)
    ln = g.integers(20, 31, (B, N)).astype(np.int32)
    for b in range(B):
        base = g.integers(0, CN - 1, 32)
        for n in range(N):
            h = base.copy()
            h[g.integers(0, 32, 3)] = g.integers(0, CN - 1, 3)
            idx[b, n, :ln[b, n]] = h[:ln[b, n]]
    return idx, ln


def scores():
    import torch
    from ishara_amd import _lib, ctc
    lib = _lib.load()
    g = np.random.default_rng(0)
    x = torch.from_numpy((g.standard_normal((B, T, CN)) * 2).astype(np.float32)).cuda()
    rows = []
    for N in NS:
        idx, ln = nbest(g, N)
        d_idx, d_ln = torch.from_numpy(idx).cuda(), torch.from_numpy(ln).cuda()
        logp = torch.empty((B, N), dtype=torch.float32, device="cuda")
        L = int(ln.max())
        tg = torch.from_numpy(np.where(idx[:, :, :L] < 0, CN - 1, idx[:, :, :L]).reshape(B * N, L).astype(np.int64)).cuda()
        tl = d_ln.reshape(B * N)
        il = torch.full((B * N,), T, dtype=torch.int32, device="cuda")

        def new():
            _lib.check(lib.ishara_ctc_score_nbest(_lib.ptr(x), B, T, CN, CN - 1, _lib.ptr(d_idx), _lib.ptr(d_ln), N, T, None, _lib.ptr(logp), None, _lib.stream()))

        def emulation():
            return ctc.ctc_loss(x.repeat_interleave(N, dim=0), tg, il, tl, blank=CN - 1, reduction="none")

        t = {k: [] for k in ("default", "hpw1", "hpw2", "hpw4", "emulation")}
        for _ in range(ROUNDS):                              # alternated: the legs share whatever else the host is doing
            for key, hpw in (("default", 0), ("hpw1", 1), ("hpw2", 2), ("hpw4", 4)):
                lib.ishara_debug_set_score_group(hpw)
                t[key] += event_ms(new, reps=15)
            lib.ishara_debug_set_score_group(0)
            t["emulation"] += event_ms(emulation, reps=6, warmup=1)
        new()
        same = bool(torch.equal(logp.reshape(-1), -emulation()))
        alloc = B * N * T * CN * 4 + int(lib.ishara_ctc_workspace_bytes(B * N, T, L))
        row = dict(N=N, lengths="20..30", label_width=L, emulation_bits_equal=same, emulation_allocates_bytes=alloc, **{k: spread(v) for k, v in t.items()})
        row["faster_by_more_than_the_spreads"] = bool(row["default"]["p90_ms"] < row["emulation"]["p10_ms"])
        row["emulation_over_new_at_median"] = row["emulation"]["median_ms"] / row["default"]["median_ms"]
        rows.append(row)
        del tg, tl, il
        torch.cuda.empty_cache()
    return rows


def rescoring():
    import torch
    from ishara_amd import _lib, rescore
    from ishara_amd.ctc_lm import CharNGramLM
    lib = _lib.load()
    g = np.random.default_rng(1)
    lm = CharNGramLM.fit([g.integers(0, CN - 1, int(g.integers(5, 31))).tolist() for _ in range(2000)], order=5, num_classes=CN)
    lm_dev = rescore.lm_to_device(lm, "cuda")
    rows = []
    for N in NS:
        idx, ln = nbest(g, N)
        d_idx, d_ln = torch.from_numpy(idx).cuda(), torch.from_numpy(ln).cuda()
        outs = (torch.empty((B, N, T), dtype=torch.int32, device="cuda"), torch.empty((B, N), dtype=torch.int32, device="cuda"),
                torch.empty((B, N), dtype=torch.float32, device="cuda"), torch.empty((B, N), dtype=torch.float32, device="cuda"),
                torch.empty((B, N), dtype=torch.int32, device="cuda"))
        for M in (1, 4):
            logps = [torch.from_numpy((-60 - 20 * g.random((B, N))).astype(np.float32)).cuda() for _ in range(M)]
            w = torch.ones(M, device="cuda")
            ptrs = rescore.pointer_array(logps)
            for name, dev in (("none", None), ("5-gram", lm_dev)):
                ts = event_ms(lambda: rescore.launch(lib, d_idx, d_ln, B, N, T, ptrs, M, w, dev, CN - 1, 0.5, 0.5, None, *outs, _lib.stream()), reps=50, warmup=5)
                rows.append(dict(N=N, M=M, lm=name, lm_states=lm_dev.S if dev is not None else 0, **spread(ts)))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("nbest_rescore_bench: no GPU: nothing here can be measured on the host")
    from ishara_amd.build import source_hash
    res = dict(workload=f"ishara_ctc_score_nbest and ishara_nbest_rescore at B {B}, T {T}, C {CN}, hypotheses of 20..30 symbols in rows of width {T}",
               source_hash=source_hash(), device=torch.cuda.get_device_name(0), score=scores(), rescore=rescoring(),
               note="event pairs around single calls with the device idle before each; the emulation is ctc.ctc_loss(reduction='none') over "
                    "logits replicated N times, replication and workspace allocation included; hpwK = K slots per wave, default = the library's "
                    "choice.  No accuracy effect is measured: there is no dataset and there are no trained weights")
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
