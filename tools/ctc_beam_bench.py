#!/usr/bin/env python3
"""CTC prefix beam search (ishara_ctc_beam_decode) cost at model scale.  Records

  * decode kernel time per batch for B = 64 / 256, T = 384, C = 60, W = 1 / 4 / 8 / 16 / 32, with and without a bigram LM (events around
    one launch on random N(0, 3^2) logits, device idle before it, median of --reps);
  * BatchedTFLiteModel at configs[4] (fp16, tools/bench_infer.MODEL_KW), batch 256: device time per graph replay and host-inclusive clips/s
    for greedy against beam 8 and beam 16 (the clips of tools/tflite_batch_bench.make_clips);
  * the host reference's (ishara_amd/ctc_beam.py) time per clip at W = 16.

The kernel times proper (without launch overhead) come from a separate `rocprofv3 --kernel-trace --stats` run of `--kernels`, which
launches every (B, W, LM) configuration KERNEL_LAUNCHES times in a fixed order; `--trace` matches the trace's ctc_beam_kernel
dispatches to the configurations by that order:

    python tools/ctc_beam_bench.py --out profiles/r6_beam_decode.json
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/ctc_beam_bench.py --kernels
    python tools/ctc_beam_bench.py --out profiles/r6_beam_decode.json --trace DIR/.../run_kernel_trace.csv
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

from tools.bench_infer import MODEL_KW  # noqa: E402


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def kernel_ms(lib, x, W, lm, reps):
    import torch
    from ishara_amd import _lib
    B, T, Cn = x.shape
    ws = torch.empty(int(lib.ishara_ctc_beam_workspace_bytes(B, T, Cn, W)), dtype=torch.uint8, device="cuda")
    idx = torch.empty((B, 1, T), dtype=torch.int32, device="cuda")
    ln = torch.empty((B, 1), dtype=torch.int32, device="cuda")
    sc = torch.empty((B, 1), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        _lib.check(lib.ishara_ctc_beam_decode(_lib.ptr(x), B, T, Cn, Cn - 1, W, 1, _lib.ptr(lm), C.c_float(0.5 if lm is not None else 0.0),
                                              C.c_float(0.5), _lib.ptr(ws), _lib.ptr(idx), _lib.ptr(ln), _lib.ptr(sc), st), "beam")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    run()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return _median(ts)


KERNEL_LAUNCHES = 5


def _configs():
    return [(B, W, lm) for B in (64, 256) for W in (1, 4, 8, 16, 32) for lm in (False, True)]


def _lm_table():
    from ishara_amd.ctc_beam import CharBigramLM
    g = np.random.default_rng(0)
    return np.asarray(CharBigramLM.fit([g.integers(0, 59, int(g.integers(3, 30))).tolist() for _ in range(500)], num_classes=60))


def kernels_run():
    """Workload for rocprofv3: KERNEL_LAUNCHES eager launches of every configuration of _configs(), in order."""
    import torch
    from ishara_amd import _lib
    lib = _lib.load()
    lm = torch.from_numpy(_lm_table()).cuda()
    g = np.random.default_rng(1)
    xs = {B: torch.from_numpy((3.0 * g.standard_normal((B, 384, 60))).astype(np.float32)).cuda() for B in (64, 256)}
    for B, W, use_lm in _configs():
        kernel_ms(lib, xs[B], W, lm if use_lm else None, KERNEL_LAUNCHES - 1)     # one warm-up + (KERNEL_LAUNCHES - 1) timed launches
    torch.cuda.synchronize()


def merge_trace(path, out):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "ctc_beam_kernel" in (r.get("Kernel_Name") or r.get("KernelName") or "")]
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r.get("Start_Timestamp")))
    cfgs = _configs()
    if len(rows) != len(cfgs) * KERNEL_LAUNCHES:
        raise SystemExit(f"{len(rows)} ctc_beam_kernel dispatches in the trace, expected {len(cfgs) * KERNEL_LAUNCHES}")
    ks = {}
    for k, (B, W, use_lm) in enumerate(cfgs):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows[k * KERNEL_LAUNCHES:(k + 1) * KERNEL_LAUNCHES]]
        ks[f"B{B}_W{W}_{'lm' if use_lm else 'no_lm'}"] = dict(median_ms=_median(d), min_ms=min(d), us_per_frame=_median(d) * 1e3 / 384)
    ks["source"] = f"rocprofv3 --kernel-trace --stats, {KERNEL_LAUNCHES} eager launches per configuration (--kernels), T=384, C=60, nbest=1"
    out["kernel_trace_ms"] = ks
    return out


def bench(args):
    import torch
    from ishara_amd import _lib, get_model
    from ishara_amd.build import source_hash
    from ishara_amd.ctc_beam import prefix_beam_search
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    from tools.tflite_batch_bench import MAX_FRAMES, make_clips, replay_ms

    lib = _lib.load()
    g = np.random.default_rng(0)
    lm = torch.from_numpy(_lm_table()).cuda()
    out = dict(workload="ishara_ctc_beam_decode, T=384, C=60, nbest=1, random N(0, 9) logits; configs[4] fp16 BatchedTFLiteModel batch 256",
               source_hash=source_hash(), timing="hip events around one launch / replay (launch overhead included), device idle before it, median")
    dec = {}
    for B in (64, 256):
        x = torch.from_numpy((3.0 * g.standard_normal((B, 384, 60))).astype(np.float32)).cuda()
        for W in (1, 4, 8, 16, 32):
            for name, l in (("no_lm", None), ("lm", lm)):
                dec[f"B{B}_W{W}_{name}"] = kernel_ms(lib, x, W, l, args.reps)
        # greedy decode on the same logits, for scale
        idx = torch.empty((B, 384), dtype=torch.int32, device="cuda")
        ln = torch.empty(B, dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            e0.record(); lib.ishara_greedy_decode(_lib.ptr(x), B, 384, 60, 59, _lib.ptr(idx), _lib.ptr(ln), st); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        g_ms = _median(ts)
        dec[f"B{B}_greedy"] = g_ms
    out["decode_ms_per_batch"] = dec

    # ---- configs[4] batched inference: greedy vs beam
    frames, off, clips, targets = make_clips()
    model = get_model(**MODEL_KW, dtype="f16", max_batch=256, seed=0)
    infer = {}
    for name, kw in (("greedy", {}), ("beam8", dict(beam_width=8)), ("beam16", dict(beam_width=16))):
        r = BatchedTFLiteModel(model, batch_size=256, max_frames=MAX_FRAMES, use_graph=True, **kw)
        r.predict_indices(clips[:512])
        ms = replay_ms(r, False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.predict_indices((frames, off))
        s = time.perf_counter() - t0
        infer[name] = dict(replay_ms=ms, device_clips_per_s=256 / ms * 1e3, host_inclusive_prepacked_clips_per_s=len(clips) / s)
        del r
        torch.cuda.empty_cache()
    for k in ("beam8", "beam16"):
        infer[k]["device_rate_vs_greedy"] = infer[k]["device_clips_per_s"] / infer["greedy"]["device_clips_per_s"]
    out["batched_tflite_b256"] = infer

    # ---- host reference
    x = (3.0 * g.standard_normal((8, 384, 60))).astype(np.float32)
    t0 = time.perf_counter()
    for b in range(x.shape[0]):
        prefix_beam_search(x[b], 16)
    host_ms = (time.perf_counter() - t0) / x.shape[0] * 1e3
    dev_ms_per_clip = dec["B256_W16_no_lm"] / 256
    out["host_reference"] = dict(ms_per_clip_W16=host_ms, device_ms_per_clip_W16_B256=dev_ms_per_clip, speedup=host_ms / dev_ms_per_clip)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
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
