#!/usr/bin/env python3
"""What model ensembling costs on the device (ishara_logits_combine, EnsembleTFLiteModel).  Records, not pass marks:

  * the fusion launch alone at B 64, T 384, C 60 for M = 2, 4, 8 in both modes: HIP-event time around one launch (device idle before
    each, REPS launches: median, min, max, 10th and 90th percentile), the bytes of the profiler's formula (M + 1) * B*T*C*4 and the
    bandwidth they give over the median.  An event pair around a launch of a few microseconds includes the launch floor: the figure is
    the cost of the call in a stream, not the kernel's own time;
  * one EnsembleTFLiteModel replay (greedy, no scoring) at M = 2 and 4 of configs[1]-sized models (dim 256, 2 + 2 blocks, T 384, bf16; 276
    input columns, which the wrapper feeds) at batch 64 against the sum of M single-model BatchedTFLiteModel replays on the same resident
    inputs, alternated in one process;
  * the device's err / bound over the case table of tests/ensemble_parity.py, per mode and input kind, with K_HOST and K.

    python tools/ensemble_bench.py --out profiles/r20_ensemble.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, T, CN = 64, 384, 60
REPS = 50
MODEL_KW = dict(dim=256, num_conv_squeeze_blocks=2, num_conv_conform_blocks=2, kernel_sizes=[11, 5, 3], num_conv_per_block=3,
                dropout_rate=0.2, num_heads=8, expansion_factor=2, transformer_kernel_size=15, input_shape=(T, 276))


def spread(ts):
    ts = np.sort(np.asarray(ts, np.float64))
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts[0]), max_ms=float(ts[-1]), p10_ms=float(np.percentile(ts, 10)),
                p90_ms=float(np.percentile(ts, 90)), reps=int(ts.size))


def event_ms(fn, reps=REPS, warmup=5):
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


def combine_alone():
    import torch
    from ishara_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    xs = [torch.randn((B, T, CN), device="cuda", generator=g) for _ in range(8)]
    out = torch.empty((B, T, CN), device="cuda")
    rows = []
    for M in (2, 4, 8):
        w = torch.full((M,), 1.0 / M, device="cuda")
        arr = (C.c_void_p * M)(*[x.data_ptr() for x in xs[:M]])
        for mode in (0, 1):
            ts = event_ms(lambda: _lib.check(lib.ishara_logits_combine(None, arr, M, B, T, CN, _lib.ptr(w), None, mode, None, _lib.ptr(out), _lib.stream())))
            nbytes = (M + 1) * B * T * CN * 4
            rec = dict(M=M, mode=("log_linear", "linear")[mode], bytes=nbytes, **spread(ts))
            rec["gb_per_s_at_median"] = nbytes / (rec["median_ms"] * 1e-3) / 1e9
            rows.append(rec)
    return rows


def replays():
    import torch
    from ishara_amd import get_model
    from ishara_amd.ensemble import EnsembleTFLiteModel
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    g = np.random.default_rng(0)
    clips = [g.standard_normal((int(n), 276)).astype(np.float32) for n in g.integers(25, 700, B)]
    models = [get_model(**MODEL_KW, dtype="bf16", max_batch=B, seed=s) for s in range(4)]
    singles = [BatchedTFLiteModel(m, batch_size=B, max_frames=1024) for m in models]
    for r in singles:
        r.predict_indices(clips)                      # captures the graphs and leaves the batch resident in device slot 0
    rows = []
    for M in (2, 4):
        ens = EnsembleTFLiteModel(models[:M], batch_size=B, max_frames=1024)
        ens.predict_indices(clips)
        t_ens, t_single = [], []
        for _ in range(4):                            # alternated: 4 rounds of REPS / 2 replays each way
            t_ens += event_ms(lambda: ens._run(0, False), reps=REPS // 2, warmup=2)
            t_single += [sum(ts) for ts in zip(*[event_ms(lambda r=r: r._run(0, False), reps=REPS // 2, warmup=2) for r in singles[:M]])]
        e, s = spread(t_ens), spread(t_single)
        rows.append(dict(M=M, batch=B, ensemble_replay=e, sum_of_single_replays=s, ensemble_over_sum=e["median_ms"] / s["median_ms"],
                         added_ms_at_median=e["median_ms"] - s["median_ms"]))
        del ens
        torch.cuda.synchronize()
    return rows


def parity():
    import torch
    import ensemble_parity as P
    from ishara_amd import _lib
    lib = _lib.load()
    groups = {}
    for c in P.cases():
        xs = [torch.from_numpy(np.array(x)).cuda() for x in c["logits"]]
        w = torch.from_numpy(np.array(c["weights"])).cuda()
        it = None if c["inv_temp"] is None else torch.from_numpy(c["inv_temp"]).cuda()
        fl = None if c["frame_len"] is None else torch.from_numpy(c["frame_len"]).cuda()
        out = torch.full((c["B"], c["T"], c["C"]), float("nan"), device="cuda")
        arr = (C.c_void_p * c["M"])(*[x.data_ptr() for x in xs])
        _lib.check(lib.ishara_logits_combine(None, arr, c["M"], c["B"], c["T"], c["C"], _lib.ptr(w), _lib.ptr(it), c["mode"], _lib.ptr(fl), _lib.ptr(out), _lib.stream()))
        key = f"mode{c['mode']}-{c['kind']}"
        groups[key] = max(groups.get(key, 0.0), P.compare(c, out.cpu().numpy()))
    return dict(K_host_recorded=P.K_HOST, K_host_measured_here=P.measure_k_host(), K=P.K, cases=len(P.cases()), device_err_over_bound=groups,
                device_err_over_bound_worst=max(groups.values()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ensemble_bench: no GPU: nothing here can be measured on the host")
    from ishara_amd.build import source_hash
    res = dict(workload=f"ishara_logits_combine at B {B}, T {T}, C {CN}; EnsembleTFLiteModel replay of configs[1]-sized bf16 models at batch {B}",
               source_hash=source_hash(), device=torch.cuda.get_device_name(0), combine_alone=combine_alone(), parity=parity(), replay=replays(),
               note="event pairs around single launches / replays with the device idle before each; no accuracy effect on real data is measured: "
                    "there is no dataset and there are no trained weights")
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
