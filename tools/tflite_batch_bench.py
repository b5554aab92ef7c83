#!/usr/bin/env python3
"""Batched raw-clip inference and device scoring at configs[4] (dim=256, 2+2 blocks, T=384, fp16 storage: tools/bench_infer.MODEL_KW).

Workload: 4096 seeded synthetic clips whose lengths are drawn uniformly from [25, 700] (an assumed distribution; real test-set lengths
are not available here), gaussian landmarks with half the frames' hand blocks NaN, random 10-32 character target phrases.  Records

  * BatchedTFLiteModel device time per graph replay at batch_size 16 / 64 / 128 / 256 (events around a replay of resident inputs, device
    idle before it, median), with and without the edit-distance launch;
  * host-inclusive clips/s at batch_size 256 for list input and pre-packed (frames, offsets) input;
  * the same process's TFLiteModel (B = 1) clips/s, device-only and host-inclusive;
  * host evaluation.mean_score time against device scoring for the same 4096 clips.

The kernel times of ishara_preprocess_batch and ishara_edit_distance come from a separate `rocprofv3 --kernel-trace --stats` run of
`--kernels` (eager launches only), merged with `--stats CSV`:

    python tools/tflite_batch_bench.py --out profiles/r5_batch_inference.json
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/tflite_batch_bench.py --kernels
    python tools/tflite_batch_bench.py --out profiles/r5_batch_inference.json --stats DIR/.../run_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_infer import HBM_PEAK_GBS, MODEL_KW  # noqa: E402

N_CLIPS, LO, HI = 4096, 25, 700
MAX_FRAMES = 704
CHARS = " !#$%&'()*+,-./0123456789:;=?@[_abcdefghijklmnopqrstuvwxyz~"
KERNEL_BATCH = 256          # batch of the --kernels run
KERNEL_LAUNCHES = 20


def make_clips(seed=0):
    g = np.random.default_rng(seed)
    lengths = g.integers(LO, HI + 1, N_CLIPS)
    off = np.zeros(N_CLIPS + 1, np.int64)
    off[1:] = np.cumsum(lengths)
    frames = g.standard_normal((int(off[-1]), 276), dtype=np.float32)
    miss = g.random(frames.shape[0]) < 0.5
    for a in range(3):
        frames[miss, a * 92:a * 92 + 42] = np.nan
    clips = [frames[off[i]:off[i + 1]] for i in range(N_CLIPS)]
    targets = ["".join(g.choice(list(CHARS), int(k))) for k in g.integers(10, 33, N_CLIPS)]
    return frames, off, clips, targets


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def replay_ms(runner, scoring, reps=20):
    """Median device time of ONE replay of slot 0 (inputs resident, host sync before each replay)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        runner._run(0, scoring)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record(); runner._run(0, scoring); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return _median(ts)


def bench(args):
    import torch
    from ishara_amd import get_model
    from ishara_amd.build import source_hash
    from ishara_amd.evaluation import mean_score
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    from ishara_amd.tflite_model import TFLiteModel
    from ishara_amd import _lib

    t0 = time.perf_counter()
    frames, off, clips, targets = make_clips()
    gen_s = time.perf_counter() - t0
    char_to_num = {c: i for i, c in enumerate(CHARS)}
    model = get_model(**MODEL_KW, dtype="f16", max_batch=256, seed=0)
    T = model.T
    out = dict(workload="configs[4] model (dim=256, 2+2 blocks, T=384, F=276, fp16 storage), inference + greedy decode + edit distance",
               source_hash=source_hash(),
               clips=dict(count=N_CLIPS, lengths=f"uniform integers in [{LO}, {HI}] (an assumed distribution)", frames=int(off[-1]),
                          mean_frames=float(off[-1] / N_CLIPS), targets="random 10-32 characters of the 59-character map",
                          landmarks="gaussian f32, hand blocks NaN on half the frames", build_s=gen_s))

    # ---- device time per replay
    per_bs = {}
    for bs in (16, 64, 128, 256):
        r = BatchedTFLiteModel(model, batch_size=bs, max_frames=MAX_FRAMES, use_graph=True)
        r.score(clips[:bs], targets[:bs], char_to_num)        # slot 0 holds this batch; both graphs of slot 0 captured
        r.predict_indices(clips[:bs])
        ms = replay_ms(r, False)
        ms_s = replay_ms(r, True)
        per_bs[str(bs)] = dict(replay_ms=ms, replay_with_scoring_ms=ms_s, us_per_clip=ms * 1e3 / bs, device_clips_per_s=bs / ms * 1e3)
        del r
        torch.cuda.empty_cache()
    out["device_replay"] = per_bs

    # ---- TFLiteModel, B = 1, same process
    single = TFLiteModel(model, max_frames=MAX_FRAMES, use_graph=True)
    x = clips[0]
    for _ in range(5):
        single(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(30):
        torch.cuda.synchronize()
        e0.record(); single._graph.replay(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    b1_ms = _median(ts)
    n1 = 256
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c in clips[:n1]:
        single(c)
    b1_host_s = (time.perf_counter() - t0) / n1
    out["tflite_b1"] = dict(replay_ms=b1_ms, device_clips_per_s=1e3 / b1_ms, host_inclusive_clips_per_s=1.0 / b1_host_s, host_clips_timed=n1)
    del single

    # ---- host-inclusive, batch_size 256, all 4096 clips
    r = BatchedTFLiteModel(model, batch_size=256, max_frames=MAX_FRAMES, use_graph=True)
    r.predict_indices(clips[:512])                               # both slots captured and warm
    host = {}
    for name, inp in (("list", clips), ("prepacked", (frames, off))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec = r.predict_indices(inp)
        s = time.perf_counter() - t0
        host[name] = dict(seconds=s, clips_per_s=N_CLIPS / s)
    host["speedup_vs_b1_host_inclusive"] = {k: host[k]["clips_per_s"] / out["tflite_b1"]["host_inclusive_clips_per_s"] for k in ("list", "prepacked")}
    out["host_inclusive_bs256"] = host
    out["device_bs256_vs_b1"] = per_bs["256"]["device_clips_per_s"] / out["tflite_b1"]["device_clips_per_s"]

    # ---- scoring: host c18 loop over strings against device edit distance
    from ishara_amd.evaluation import make_num_to_char
    from ishara_amd.tflite_batch import apply_fallback
    n2c = make_num_to_char(char_to_num)
    preds = ["".join(n2c.get(int(s), "") for s in apply_fallback(d)) for d in dec]
    t0 = time.perf_counter()
    host_mean = mean_score(preds, targets)
    host_s = time.perf_counter() - t0
    res = r.score((frames, off), targets, char_to_num)
    # device scoring time: the edit-distance launch alone on the resident decodes of the last batch, times the batch count
    d = r._d_in[0]
    lib = model._lib
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(20):
        torch.cuda.synchronize()
        e0.record()
        _lib.check(lib.ishara_edit_distance(_lib.ptr(r._idx), _lib.ptr(r._len), 256, T, _lib.ptr(r._tgt(d)), r.L, _lib.ptr(r._dist),
                                            _lib.ptr(r._tlen), torch.cuda.current_stream().cuda_stream), "ishara_edit_distance")
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ed_ms = _median(ts)
    nb = (N_CLIPS + 255) // 256
    out["scoring"] = dict(host_mean_score_s=host_s, host_ms_per_1000_clips=host_s / N_CLIPS * 1e6,
                          device_edit_distance_ms_per_batch256=ed_ms, device_ms_all_clips=ed_ms * nb,
                          device_speedup=host_s * 1e3 / (ed_ms * nb), mean_score_equal=bool(res["mean_score"] == host_mean),
                          mean_score=res["mean_score"], mean_prediction_len=float(np.mean([len(p) for p in preds])))
    out["targets"] = dict(device_bs256_vs_b1=">= 20x", device_scoring_vs_host=">= 50x", preprocess_batch_us="<= 80")
    return out


def kernels_run():
    """Workload for rocprofv3: eager launches of the batch-256 sequence, edit distance included."""
    import torch
    from ishara_amd import get_model
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    frames, off, clips, targets = make_clips()
    char_to_num = {c: i for i, c in enumerate(CHARS)}
    model = get_model(**MODEL_KW, dtype="f16", max_batch=256, seed=0)
    r = BatchedTFLiteModel(model, batch_size=KERNEL_BATCH, max_frames=MAX_FRAMES, use_graph=False)
    r.score(clips[:KERNEL_BATCH], targets[:KERNEL_BATCH], char_to_num)
    for _ in range(KERNEL_LAUNCHES - 1):
        r._run(0, True)
    torch.cuda.synchronize()


def merge_stats(path, out):
    rows = list(csv.DictReader(open(path)))
    n = int(np.random.default_rng(0).integers(LO, HI + 1, N_CLIPS)[:KERNEL_BATCH].sum())     # make_clips' first draw
    T = MODEL_KW["input_shape"][0]
    by = {"preprocess_batch_kernel": n * 276 * 4 + KERNEL_BATCH * T * 276 * 4,
          "edit_distance_kernel": KERNEL_BATCH * (T * 4 + 4 + 64 * 4 + 8)}
    ks = {}
    for row in rows:
        name = row.get("Name") or row.get("KernelName") or ""
        for k, b in by.items():
            if k in name:
                avg_ns = float(row.get("AverageNs") or row.get("AverageNs ") or 0)
                ks[k] = dict(calls=int(row.get("Calls", 0)), avg_us=avg_ns / 1e3, min_us=float(row.get("MinNs", 0)) / 1e3,
                             bytes=b, GBps=b / avg_ns if avg_ns else None, hbm_floor_us=b / (HBM_PEAK_GBS * 1e3))
    ks["batch"] = KERNEL_BATCH
    ks["raw_frames_in_batch"] = n
    ks["source"] = "rocprofv3 --kernel-trace --stats, eager launches of the batch-256 sequence (--kernels)"
    out["kernels"] = ks
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true", help="only run the rocprofv3 workload")
    ap.add_argument("--stats", default=None, help="merge a rocprofv3 kernel_stats.csv into --out (no GPU)")
    a = ap.parse_args()
    if a.kernels:
        kernels_run()
        sys.exit(0)
    if a.stats:
        res = merge_stats(a.stats, json.load(open(a.out)))
    else:
        res = bench(a)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
