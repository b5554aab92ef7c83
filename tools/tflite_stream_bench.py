#!/usr/bin/env python3
"""Streaming recognition at configs[4] (dim=256, 2+2 blocks, T=384, fp16 storage: tools/bench_infer.MODEL_KW), 16 and 64 sessions.

Workload: the first S synthetic clips of tools/tflite_batch_bench.py (lengths uniform in [25, 700], hand blocks NaN on half the frames), one
clip per session, fed ONE FRAME PER TICK: at tick t session s receives frame t of its clip while it has one, nothing afterwards (no finish:
a session keeps its whole clip, so at the last tick the S sessions hold the S clips).  Records, per S,

  * the device time of every real tick (events around the graph replay inside push) and the host-inclusive push latency;
  * at a few fill levels, alternated in the same process on the same stored frames: one StreamingTFLiteModel replay (staging emptied, so
    that the replay stores nothing and can be repeated) against one BatchedTFLiteModel replay at batch_size = S, and their ratio.

Nothing is asserted and no bound is fixed: the expectation is tick = batched replay + the append and agree kernels.  The kernel times come
from a separate rocprofv3 run of `--kernels` (eager launches: the clips preloaded in chunks, then one-frame ticks, then the batched sequence
on the same stored frames), of which only each kernel's last dispatches (the one-frame ticks / the batched launches) are read:

    python tools/tflite_stream_bench.py --out profiles/r16_stream.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/tflite_stream_bench.py --kernels
    python tools/tflite_stream_bench.py --out profiles/r16_stream.json --trace DIR/.../run_kernel_trace.csv
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

from tools.bench_infer import MODEL_KW  # noqa: E402
from tools.tflite_batch_bench import make_clips  # noqa: E402

WINDOW = 1024
MEASURE_AT = (100, 300, 700)      # ticks after which the replays are compared (700: every clip is complete)
AB_REPS = 9
KERNEL_S, KERNEL_TICKS, KERNEL_CHUNK = 64, 40, 64
KERNELS = ("stream_append_kernel", "preprocess_sessions_kernel", "stream_agree_kernel", "preprocess_batch_kernel")


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))]


def _timed(fn, e0, e1):
    import torch
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stored_clips(m):
    n = m._counters[:, 0].cpu().numpy()
    raw = m._raw.cpu().numpy()
    return [raw[s, :int(n[s])].copy() for s in range(m.sessions)]


def bench_sessions(model, clips, S):
    import torch
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    from ishara_amd.tflite_stream import StreamingTFLiteModel
    m = StreamingTFLiteModel(model, sessions=S, window=WINDOW, use_graph=True)
    b = BatchedTFLiteModel(model, batch_size=S, max_frames=WINDOW, use_graph=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    replay = m._tick

    def timed_tick():
        e0.record(); replay(); e1.record()
    m._tick = timed_tick
    tick_ms, push_ms, points, finals = [], [], [], 0
    for t in range(max(len(c) for c in clips)):
        frames = {s: c[t:t + 1] for s, c in enumerate(clips) if t < len(c)}
        t0 = time.perf_counter()
        res = m.push(frames)
        push_ms.append((time.perf_counter() - t0) * 1e3)
        tick_ms.append(e0.elapsed_time(e1))
        finals += sum(r.final for r in res)
        if t + 1 in MEASURE_AT or t + 1 == max(len(c) for c in clips):
            stored = stored_clips(m)
            b.predict_indices(stored)                              # slot 0 of the batched runner holds the same frames
            m._d_in[:m._frames_at].zero_()                         # no frames, no flags: the replay below changes no state
            a_ms, b_ms = [], []
            for _ in range(AB_REPS):
                a_ms.append(_timed(replay, e0, e1))
                b_ms.append(_timed(lambda: b._run(0, False), e0, e1))
            sa, sb = _median(a_ms), _median(b_ms)
            points.append(dict(tick=t + 1, frames_stored=int(sum(len(x) for x in stored)), stream_replay_ms=sa, batched_replay_ms=sb,
                               stream_minus_batched_us=(sa - sb) * 1e3, ratio=sa / sb))
    tail = tick_ms[-100:]
    return dict(sessions=S, ticks=len(tick_ms), finals_seen=finals,
                tick_device_ms=dict(median=_median(tick_ms), p95=_pct(tick_ms, 0.95), median_last_100=_median(tail), max=max(tick_ms)),
                push_host_inclusive_ms=dict(median=_median(push_ms), p95=_pct(push_ms, 0.95), median_last_100=_median(push_ms[-100:])),
                replay_vs_batched=points)


def bench(args):
    from ishara_amd import get_model
    from ishara_amd.build import source_hash
    _, _, clips, _ = make_clips()
    model = get_model(**MODEL_KW, dtype="f16", max_batch=64, seed=0)
    out = dict(workload="configs[4] model (dim=256, 2+2 blocks, T=384, F=276, fp16 storage), streaming: one frame per session and tick, greedy decode",
               source_hash=source_hash(), window=WINDOW,
               clips="the first S clips of tools/tflite_batch_bench.make_clips (lengths uniform in [25, 700], hand blocks NaN on half the frames)",
               method="tick_device_ms: events around the replay inside push, every tick; replay_vs_batched: alternated replays on the same stored "
                      f"frames, device idle before each, median of {AB_REPS}; the stream replay of that comparison appends no frame",
               not_measured="recognition quality of partial clips; agree / idle_frames / min_active_frames / window are untuned defaults")
    out["sessions"] = {str(S): bench_sessions(model, clips[:S], S) for S in (16, 64)}
    return out


def kernels_run():
    """Workload for rocprofv3: eager launches.  The clips go in in chunks of 64 frames, then KERNEL_TICKS one-frame ticks, then as many
    launches of the batched sequence on the same stored frames."""
    import torch
    from ishara_amd import get_model
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    from ishara_amd.tflite_stream import StreamingTFLiteModel
    _, _, clips, _ = make_clips()
    clips = clips[:KERNEL_S]
    model = get_model(**MODEL_KW, dtype="f16", max_batch=KERNEL_S, seed=0)
    m = StreamingTFLiteModel(model, sessions=KERNEL_S, window=WINDOW, max_push=KERNEL_CHUNK, use_graph=False)
    b = BatchedTFLiteModel(model, batch_size=KERNEL_S, max_frames=WINDOW, use_graph=False)
    body = [c[:len(c) - KERNEL_TICKS] if len(c) > KERNEL_TICKS else c[:0] for c in clips]
    for t0 in range(0, max(len(c) for c in body), KERNEL_CHUNK):
        m.push({s: c[t0:t0 + KERNEL_CHUNK] for s, c in enumerate(body) if t0 < len(c)})
    for t in range(KERNEL_TICKS):
        m.push({s: c[len(body[s]) + t:len(body[s]) + t + 1] for s, c in enumerate(clips) if len(body[s]) + t < len(c)})
    b.predict_indices(stored_clips(m))
    for _ in range(KERNEL_TICKS - 1):
        b._run(0, False)
    torch.cuda.synchronize()


def merge_trace(path, out):
    """Median / min of each kernel's last KERNEL_TICKS dispatches in a rocprofv3 kernel trace."""
    rows = list(csv.DictReader(open(path)))
    ks = {}
    for k in KERNELS:
        d = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if k in r["Kernel_Name"])
        us = [(e - s) / 1e3 for s, e in d[-KERNEL_TICKS:]]
        if us:
            ks[k] = dict(dispatches_in_trace=len(d), dispatches_read=len(us), median_us=_median(us), min_us=min(us), max_us=max(us))
    ks["sessions"] = KERNEL_S
    ks["source"] = (f"rocprofv3 --kernel-trace, eager launches (--kernels): each kernel's last {KERNEL_TICKS} dispatches, i.e. the one-frame ticks on "
                    "whole clips and the batched launches on the same stored frames")
    if all(k in ks for k in KERNELS[:3]):
        ks["append_plus_agree_us"] = ks["stream_append_kernel"]["median_us"] + ks["stream_agree_kernel"]["median_us"]
    out["kernels"] = ks
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true", help="only run the rocprofv3 workload")
    ap.add_argument("--trace", default=None, help="merge a rocprofv3 kernel_trace.csv into --out (no GPU)")
    a = ap.parse_args()
    if a.kernels:
        kernels_run()
        sys.exit(0)
    if a.trace:
        res = merge_trace(a.trace, json.load(open(a.out)))
    else:
        res = bench(a)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
