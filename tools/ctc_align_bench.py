#!/usr/bin/env python3
"""CTC forced alignment (ishara_ctc_align) cost at model scale, next to its yardstick.  Records, at T = 384, C = 60, L = 64 and B = 256 / 64
(random N(0, 3^2) logits, label lengths uniform in 8 .. 64):

  * the alignment launch and, in the same process on the same inputs, the loss-only launch of ishara_ctc_loss (dlogits = NULL): the same
    lattice with a heavier per-frame chain (log-sum-exp against compare / select) but no backtrace.  Events around one launch, device idle
    before it, median of --reps;
  * the host reference's (ishara_amd/ctc_align.py viterbi_align) time per clip.

The kernel times proper (without launch overhead) come from a separate `rocprofv3 --kernel-trace --stats` run of `--kernels`, which
launches every configuration KERNEL_LAUNCHES times in a fixed order; `--trace` matches the trace's dispatches to them by that order:

    python tools/ctc_align_bench.py --out profiles/r7_ctc_align.json
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/ctc_align_bench.py --kernels
    python tools/ctc_align_bench.py --out profiles/r7_ctc_align.json --trace DIR/.../run_kernel_trace.csv
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, CN, L = 384, 60, 64
BATCHES = (256, 64)
KERNEL_LAUNCHES = 5
MARGIN = 1.5          # the alignment may take this many times the loss-only launch: the backtrace is a second serial chain


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def make_inputs(B):
    g = np.random.default_rng(B)
    x = (3.0 * g.standard_normal((B, T, CN))).astype(np.float32)
    y = np.full((B, L), CN - 1, np.int64)
    for b in range(B):
        n = int(g.integers(8, L + 1))
        y[b, :n] = g.integers(0, CN - 1, n)
    return x, y


def _timed(run, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    run()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return _median(ts)


def launches(lib, x, y):
    """(align, loss-only) launch closures on device copies of x, y"""
    import torch
    from ishara_amd import _lib
    B = x.shape[0]
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(max(int(lib.ishara_ctc_align_workspace_bytes(B, T, L)), 16), dtype=torch.uint8, device="cuda")
    fp = torch.empty((B, T), dtype=torch.int32, device="cuda")
    sp = [torch.empty((B, L), dtype=torch.int32, device="cuda") for _ in range(2)]
    cf = torch.empty((B, L), dtype=torch.float32, device="cuda")
    sc = torch.empty(B, dtype=torch.float32, device="cuda")
    lws = torch.empty(int(lib.ishara_ctc_workspace_bytes(B, T, L)), dtype=torch.uint8, device="cuda")
    nll = torch.empty(B, dtype=torch.float32, device="cuda")

    def align():
        _lib.check(lib.ishara_ctc_align(_lib.ptr(x), _lib.ptr(y), B, T, CN, L, CN - 1, _lib.ptr(ws), _lib.ptr(fp), _lib.ptr(sp[0]), _lib.ptr(sp[1]),
                                        _lib.ptr(cf), _lib.ptr(sc), st), "ishara_ctc_align")

    def loss():
        _lib.check(lib.ishara_ctc_loss(_lib.ptr(x), _lib.ptr(y), B, T, CN, L, CN - 1, _lib.ptr(nll), None, C.c_float(1.0), _lib.ptr(lws), st), "ishara_ctc_loss")
    return align, loss


def kernels_run():
    """Workload for rocprofv3: per batch size KERNEL_LAUNCHES launches of the alignment, then of the loss-only kernel."""
    import torch
    from ishara_amd import _lib
    lib = _lib.load()
    for B in BATCHES:
        for run in launches(lib, *make_inputs(B)):
            for _ in range(KERNEL_LAUNCHES):
                run()
                torch.cuda.synchronize()


def merge_trace(path, out):
    import csv
    rows = list(csv.DictReader(open(path)))
    name = lambda r: r.get("Kernel_Name") or r.get("KernelName") or ""
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r.get("Start_Timestamp")))
    ks = {}
    for kernel, key in (("ctc_align_kernel", "align"), ("ctc_kernel", "loss_only")):
        mine = [r for r in rows if kernel in name(r)]
        if len(mine) != len(BATCHES) * KERNEL_LAUNCHES:
            raise SystemExit(f"{len(mine)} {kernel} dispatches in the trace, expected {len(BATCHES) * KERNEL_LAUNCHES}")
        for k, B in enumerate(BATCHES):
            d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in mine[k * KERNEL_LAUNCHES:(k + 1) * KERNEL_LAUNCHES]]
            ks[f"B{B}_{key}"] = dict(median_ms=_median(d), min_ms=min(d), us_per_frame=_median(d) * 1e3 / T)
    for B in BATCHES:
        r = ks[f"B{B}_align"]["median_ms"] / ks[f"B{B}_loss_only"]["median_ms"]
        ks[f"B{B}_ratio"] = dict(align_over_loss_only=r, margin=MARGIN, verdict="met" if r <= MARGIN else "missed")
    ks["source"] = f"rocprofv3 --kernel-trace --stats, {KERNEL_LAUNCHES} eager launches per configuration (--kernels), T={T}, C={CN}, L={L}"
    out["kernel_trace_ms"] = ks
    return out


def bench(args):
    from ishara_amd import _lib
    from ishara_amd.build import source_hash
    from ishara_amd.ctc_align import viterbi_align
    lib = _lib.load()
    out = dict(workload=f"ishara_ctc_align against ishara_ctc_loss with dlogits = NULL, T={T}, C={CN}, L={L}, random N(0, 9) logits, label lengths 8..{L}",
               source_hash=source_hash(), timing="hip events around one launch (launch overhead included), device idle before it, median")
    ms = {}
    for B in BATCHES:
        x, y = make_inputs(B)
        align, loss = launches(lib, x, y)
        ms[f"B{B}_align"] = _timed(align, args.reps)
        ms[f"B{B}_loss_only"] = _timed(loss, args.reps)
        ms[f"B{B}_align_over_loss_only"] = ms[f"B{B}_align"] / ms[f"B{B}_loss_only"]
    out["launch_ms_per_batch"] = ms
    x, y = make_inputs(8)
    t0 = time.perf_counter()
    viterbi_align(x, y, CN - 1)
    host_ms = (time.perf_counter() - t0) / 8 * 1e3
    dev = ms["B256_align"] / 256
    out["host_reference"] = dict(ms_per_clip=host_ms, device_ms_per_clip_B256=dev, speedup=host_ms / dev)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels", action="store_true", help="only run the rocprofv3 workload")
    ap.add_argument("--trace", default=None, help="merge a rocprofv3 kernel_trace.csv into --out (no GPU)")
    a = ap.parse_args()
    if a.kernels:
        kernels_run()
        sys.exit(0)
    res = merge_trace(a.trace, json.load(open(a.out))) if a.trace else bench(a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
