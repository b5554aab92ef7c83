#!/usr/bin/env python3
"""What the error breakdown of BatchedTFLiteModel.score costs, at configs[4] (dim=256, 2+2 blocks, T=384, fp16 storage), batch 256, on the
4096 synthetic clips of tools/tflite_batch_bench.py (lengths uniform in [25, 700], random 10-32 character targets).  Records

  * device time of one `score` graph replay with and without `breakdown` (events around replays of resident inputs, device idle before
    each, median), in one process;
  * the alignment launch alone next to the edit-distance launch alone on the same resident decodes (events, median);
  * the host `evaluation.error_report` time on the same decodes, and that the device report equals it.

The kernel times of edit_alignment_kernel and edit_distance_kernel come from a separate `rocprofv3 --kernel-trace --stats` run of
`--kernels` (eager launches only), merged with `--stats CSV`:

    python tools/error_report_bench.py --out profiles/r14_error_report.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/error_report_bench.py --kernels
    python tools/error_report_bench.py --out profiles/r14_error_report.json --stats DIR/.../run_kernel_stats.csv
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
from tools.tflite_batch_bench import CHARS, MAX_FRAMES, N_CLIPS, _median, make_clips  # noqa: E402

BATCH = 256
KERNEL_LAUNCHES = 20
HOST_CLIPS = 512            # the host loop is timed on this many clips and scaled (it is linear in the clip count)


def replay_ms(runner, breakdown, reps=20):
    """Median device time of ONE scoring replay of slot 0 (inputs resident, host sync before each replay)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        runner._run(0, True, breakdown)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record(); runner._run(0, True, breakdown); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return _median(ts)


def launch_ms(fn, reps=20):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return _median(ts)


def bench():
    import torch
    from ishara_amd import _lib, get_model
    from ishara_amd.build import source_hash
    from ishara_amd.evaluation import error_report
    from ishara_amd.tflite_batch import BatchedTFLiteModel, apply_fallback, encode_phrase

    frames, off, clips, targets = make_clips()
    char_to_num = {c: i for i, c in enumerate(CHARS)}
    model = get_model(**MODEL_KW, dtype="f16", max_batch=BATCH, seed=0)
    r = BatchedTFLiteModel(model, batch_size=BATCH, max_frames=MAX_FRAMES, use_graph=True)
    out = dict(workload="configs[4] model (dim=256, 2+2 blocks, T=384, F=276, fp16 storage), score() at batch 256 with and without breakdown",
               source_hash=source_hash(), clips=N_CLIPS, batch=BATCH)

    # ---- the whole test set each way, alternated (host-inclusive, median of 3): equal scores, and the report against the host loop
    plain = r.score((frames, off), targets, char_to_num)
    res = r.score((frames, off), targets, char_to_num, breakdown=True)      # every graph captured before timing
    times = {False: [], True: []}
    for _ in range(3):
        for brk in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.score((frames, off), targets, char_to_num, breakdown=brk)
            times[brk].append(time.perf_counter() - t0)
    plain_s, brk_s = _median(times[False]), _median(times[True])
    dec = r.predict_indices((frames, off))
    enc = np.stack([encode_phrase(t, char_to_num, r.L) for t in targets])
    t0 = time.perf_counter()
    host = error_report([apply_fallback(d) for d in dec[:HOST_CLIPS]], enc[:HOST_CLIPS], max_len=r.L)
    host_s = (time.perf_counter() - t0) * N_CLIPS / HOST_CLIPS
    part = r.score(clips[:HOST_CLIPS], targets[:HOST_CLIPS], char_to_num, breakdown=True)
    rep = res["report"]
    out["report"] = dict(equal_to_host_on_first_clips=bool(part["report"] == host), host_clips_compared=HOST_CLIPS,
                         mean_score_unchanged=bool(res["mean_score"] == plain["mean_score"]), matches=rep.matches,
                         substitutions=rep.substitutions, deletions=rep.deletions, insertions=rep.insertions,
                         mean_prediction_len=float(np.mean([len(apply_fallback(d)) for d in dec])))
    out["host_inclusive"] = dict(score_s=plain_s, score_breakdown_s=brk_s, host_error_report_s=host_s,
                                 host_error_report_note=f"timed on {HOST_CLIPS} clips, scaled to {N_CLIPS}")

    # ---- device time per replay, slot 0 resident (the last whole batch the calls above left there)
    r.score(clips[:BATCH], targets[:BATCH], char_to_num, breakdown=True)
    r.score(clips[:BATCH], targets[:BATCH], char_to_num)
    ms0, ms1 = replay_ms(r, False), replay_ms(r, True)
    out["device_replay"] = dict(score_ms=ms0, score_breakdown_ms=ms1, added_ms=ms1 - ms0, added_fraction=(ms1 - ms0) / ms0)

    # ---- the two launches alone on the resident decodes
    lib, d, k = model._lib, r._d_in[0], r._breakdown_buffers()
    st = torch.cuda.current_stream().cuda_stream
    ed_ms = launch_ms(lambda: _lib.check(lib.ishara_edit_distance(_lib.ptr(r._idx), _lib.ptr(r._len), BATCH, r.T, _lib.ptr(r._tgt(d)), r.L,
                                                                  _lib.ptr(r._dist), _lib.ptr(r._tlen), st), "ishara_edit_distance"))
    al_ms = launch_ms(lambda: r._launch_alignment(0, BATCH))
    nb = (N_CLIPS + BATCH - 1) // BATCH
    out["launches"] = dict(edit_distance_ms_per_batch256=ed_ms, edit_alignment_ms_per_batch256=al_ms, ratio=al_ms / ed_ms,
                           edit_alignment_ms_all_clips=al_ms * nb, host_over_device=host_s * 1e3 / (al_ms * nb),
                           workspace_bytes=int(lib.ishara_edit_alignment_workspace_bytes(BATCH, r.T)))
    return out


def kernels_run():
    """Workload for rocprofv3: eager launches of the batch-256 scoring sequence with the breakdown."""
    import torch
    from ishara_amd import get_model
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    frames, off, clips, targets = make_clips()
    char_to_num = {c: i for i, c in enumerate(CHARS)}
    model = get_model(**MODEL_KW, dtype="f16", max_batch=BATCH, seed=0)
    r = BatchedTFLiteModel(model, batch_size=BATCH, max_frames=MAX_FRAMES, use_graph=False)
    r.score(clips[:BATCH], targets[:BATCH], char_to_num, breakdown=True)
    for _ in range(KERNEL_LAUNCHES - 1):
        r._run(0, True, True)
    torch.cuda.synchronize()


def merge_stats(path, out):
    ks = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        for k in ("edit_alignment_kernel", "edit_distance_kernel"):
            if k in name:
                ks[k] = dict(calls=int(row.get("Calls", 0)), avg_us=float(row.get("AverageNs") or 0) / 1e3, min_us=float(row.get("MinNs", 0)) / 1e3,
                             max_us=float(row.get("MaxNs", 0)) / 1e3)
    if "edit_alignment_kernel" in ks and "edit_distance_kernel" in ks and ks["edit_distance_kernel"]["avg_us"]:
        ks["ratio"] = ks["edit_alignment_kernel"]["avg_us"] / ks["edit_distance_kernel"]["avg_us"]
    ks["batch"] = BATCH
    ks["source"] = "rocprofv3 --kernel-trace --stats, eager launches of the batch-256 scoring sequence with breakdown (--kernels)"
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
    res = merge_stats(a.stats, json.load(open(a.out))) if a.stats else bench()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
