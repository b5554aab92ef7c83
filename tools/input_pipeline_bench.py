#!/usr/bin/env python3
"""Input pipeline at configs[1] (B=256, T=384, F=224 hands_lips_xy, bf16 model): the host path of ishara_amd/data.py
(BatchAdapter over an augmenting ClipDataset) against the device path (DeviceClipStore + DeviceBatchAdapter, one
ishara_clip_batch launch per batch), and a train_on_batch loop fed by each.  Synthetic seeded store: 4096 clips, lengths uniform
in [64, 640] (an assumed distribution), gaussian landmarks.  Prints one JSON object; --out also writes it to a file.

    python tools/input_pipeline_bench.py --out profiles/r4_input_pipeline.json
"""
import argparse
import ctypes as C
import itertools
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


class NonEmptyShift(random.Random):
    """random.Random whose shift draw (randint(-10, 10)) redraws 0.  A shift of 0 empties the clip (the reference's `[:0]`) and a
    following dropout draw then raises, as in the reference, on ~1 % of clips: an epoch over 4096 clips would not finish."""

    def randint(self, a, b):
        v = super().randint(a, b)
        while (a, b) == (-10, 10) and v == 0:
            v = super().randint(a, b)
        return v


class SyntheticClips:
    def __init__(self, n_clips, lo, hi, seed):
        self.lengths = np.random.default_rng(seed).integers(lo, hi + 1, n_clips)
        self.seed = seed

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, i):
        g = np.random.default_rng((self.seed, i))
        n = int(self.lengths[i])
        return g.standard_normal((n, 124, 3), dtype=np.float32), list(g.integers(0, 59, int(g.integers(8, 32))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=384)
    ap.add_argument("--host-batches", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed loop")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the premade / device-adapter loops")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from ishara_amd import _lib, get_model
    from ishara_amd import data as D
    sys.path.insert(0, ROOT)
    from bench import CONFIGS

    B, T, layout = args.batch, args.frames, "hands_lips_xy"
    F = 224
    dev = "cuda:0"
    clips = SyntheticClips(args.clips, 64, 640, seed=0)
    out = {"workload": f"configs[1] input: B={B} T={T} F={F} ({layout}), augment on",
           "store": {"clips": args.clips, "lengths": "uniform integers in [64, 640] (assumed distribution)", "landmarks": "gaussian f32",
                     "rng": "NonEmptyShift (random.Random with the emptying shift-of-0 draw redrawn)"}}

    # ---- host path: BatchAdapter over an augmenting ClipDataset (data_loader.py restated in numpy, one clip at a time)
    host = D.BatchAdapter(D.ClipDataset(clips, T, augment=True, rng=NonEmptyShift(1)), B, layout=layout)
    it = iter(host)
    t0 = time.perf_counter()
    for _ in range(args.host_batches):
        next(it)
    out["host_path_ms_per_batch"] = (time.perf_counter() - t0) / args.host_batches * 1e3
    out["host_path_batches"] = args.host_batches

    # ---- device store
    t0 = time.perf_counter()
    store = D.DeviceClipStore(clips, dev)
    torch.cuda.synchronize()
    out["store"].update(frames=int(store.n_frames), bytes=int(store.raw.numel()) * 4, build_s=time.perf_counter() - t0)

    # ---- host cost of the device path: draws + table for one batch
    rng = NonEmptyShift(2)
    idx = np.arange(B)
    tab = np.zeros(B, D.CLIP_AUG_DTYPE)
    reps = 20
    t0 = time.perf_counter()
    for r in range(reps):
        draws = [D.draw_augmentation(n, rng) for n in store.lengths[idx + r * B % (args.clips - B)]]
        D.fill_clip_table(tab, store.offsets[idx], draws)
    out["draws_table_host_ms_per_batch"] = (time.perf_counter() - t0) / reps * 1e3

    # ---- the kernel alone on one batch's table, device events
    draws = [D.draw_augmentation(n, rng) for n in store.lengths[idx]]
    D.fill_clip_table(tab, store.offsets[idx], draws)
    dtab = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    x = torch.empty((B, T, F), dtype=torch.float32, device=dev)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        _lib.check(lib.ishara_clip_batch(_lib.ptr(store.raw), _lib.ptr(dtab), B, T, 1, _lib.ptr(x), stream), "ishara_clip_batch")
    for _ in range(5):
        launch()
    n_launch = 50
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n_launch):
        launch()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / n_launch * 1e3
    # algorithmic bytes: every non-zero output frame reads its raw frame once (124*3 f32), plus the write of x
    frames_read = 0
    for d in draws:
        for t in range(T):
            L2 = d.L2
            j = (L2 - 1 if t == T - 1 else int(t * ((L2 - 1) / (T - 1)))) if L2 > T else (t if t < L2 else -1)
            k = j + (d.shift or 0)
            frames_read += j >= 0 and 0 <= k < d.L1
    rd, wr = frames_read * 124 * 3 * 4, B * T * F * 4
    out["clip_batch_kernel"] = {"us": us, "launches_timed": n_launch, "read_bytes": rd, "write_bytes": wr,
                                "GBps": (rd + wr) / us * 1e-3, "hbm_floor_us": (rd + wr) / (HBM_PEAK_GBS * 1e3),
                                "target_us": 100.0, "note": "same table every launch: the clips stay in L2 / the Infinity Cache between launches"}

    # ---- train_on_batch loops: premade device batch vs DeviceBatchAdapter, alternated in this process
    cfg = CONFIGS[2]
    model = get_model(**cfg["kw"], dtype="bf16", max_batch=B, device=dev, seed=0)
    model.optimizer.learning_rate = 1e-3
    ad = D.DeviceBatchAdapter(store, B, T, layout=layout, shuffle=True, seed=3, rng=NonEmptyShift(3), drop_last=True)
    stream_batches = itertools.chain.from_iterable(itertools.repeat(ad))
    xp, yp = next(stream_batches)
    xp, yp = xp.clone(), yp.clone()

    def premade():
        return model.train_on_batch(xp, yp)

    def adapter():
        xb, yb = next(stream_batches)
        return model.train_on_batch(xb, yb)

    for fn in (premade, adapter, premade, adapter):
        fn()
    torch.cuda.synchronize()
    times = {"premade": [], "device_adapter": []}
    for _ in range(args.rounds):
        for name, fn in (("premade", premade), ("device_adapter", adapter)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out["train_loop_ms_per_step"] = {k: {"mean": float(np.mean(v)), "runs": v} for k, v in times.items()}
    out["train_loop_ms_per_step"]["adapter_over_premade"] = float(np.mean(times["device_adapter"]) / np.mean(times["premade"]))
    out["train_loop_ms_per_step"]["steps_per_run"] = args.steps
    out["loss_finite"] = bool(np.isfinite(float(loss.item())))
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
