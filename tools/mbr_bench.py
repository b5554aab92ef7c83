#!/usr/bin/env python3
"""What minimum-Bayes-risk decoding costs on the device (ishara_mbr_select, the wrappers' mbr_nbest).  Records, not pass marks:

  * the selection launch alone at B 64 for N = 8, 16, 32, 64 hypotheses of 20 to 30 symbols (T 384, C 60, mode 1): HIP-event time around
    one launch (device idle before each, REPS launches: median, min, max, 10th and 90th percentile).  An event pair around a launch of a
    few microseconds includes the launch floor: the figure is the cost of the call in a stream, not the kernel's own time;
  * beside it the beam search with the same nbest at T 384, W 32 on noisy synthetic logits (N 64 exceeds the beam's width of 32 and has no
    such row);
  * one BatchedTFLiteModel replay at batch 64 of a configs[1]-sized bf16 model (dim 256, 2 + 2 blocks, T 384) with beam_width 16, without
    and with mbr_nbest 8, alternated in one process.  --plain-only measures the first alone and uses nothing newer than the beam
    wrapper, so the same file runs on an older checkout for a figure of the parent commit;
  * a SYNTHETIC accuracy figure: the mean normalised score of the beam's top-1 and of the MBR choice on logits built from noisy targets.
    No effect on real data can be measured: there is no dataset and there are no trained weights.

    python tools/mbr_bench.py --out profiles/r21_mbr.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, CN, W = 64, 384, 60, 32
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


def noisy_logits(seed, nclips, frames, noise):
    """confident alignments of random phrases plus N(0, noise^2) on every logit: (logits float32 [nclips, frames, C], the phrases)"""
    g = np.random.default_rng(seed)
    x, phrases = np.zeros((nclips, frames, CN)), []
    for b in range(nclips):
        t, lab, prev = 0, [], None
        while t < frames - 8:
            n = int(g.integers(4, 16))
            c = CN - 1 if (prev not in (None, CN - 1) and g.random() < 0.5) else int(g.integers(0, CN - 1))
            if c == prev:
                c = CN - 1
            x[b, t:min(t + n, frames - 8), c] += 4.0
            if c != CN - 1:
                lab.append(c)
            prev, t = c, t + n
        x[b, frames - 8:, CN - 1] += 4.0
        phrases.append(lab)
    return (x + noise * g.standard_normal(x.shape)).astype(np.float32), phrases


def select_alone():
    import torch
    from ishara_amd import _lib, mbr
    lib = _lib.load()
    g = np.random.default_rng(0)
    rows = []
    for N in (8, 16, 32, 64):
        idx = np.full((B, N, T), -1, np.int32)
        ln = g.integers(20, 31, (B, N)).astype(np.int32)
        for b in range(B):
            base = g.integers(0, CN - 1, 32)
            for n in range(N):
                h = base.copy()
                h[g.integers(0, 32, 3)] = g.integers(0, CN - 1, 3)
                idx[b, n, :ln[b, n]] = h[:ln[b, n]]
        sc = -np.sort(g.random((B, N)) * 8, axis=1).astype(np.float32)
        d = [torch.from_numpy(a).cuda() for a in (idx, ln, sc)]
        out = (torch.empty((B, T), dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))
        ts = event_ms(lambda: mbr.launch(lib, d[0], d[1], d[2], None, None, B, N, T, CN, 1, out[0], out[1], out[2], None, None, None, None, _lib.stream()))
        rows.append(dict(N=N, pairs=N * (N - 1) // 2, lengths="20..30", **spread(ts)))
    return rows


def beam_alone():
    import torch
    from ishara_amd import _lib, ctc_beam
    lib = _lib.load()
    x = torch.from_numpy(noisy_logits(1, B, T, 1.5)[0]).cuda()
    ws = torch.empty(max(ctc_beam.workspace_bytes(lib, B, T, CN, W), 4), dtype=torch.uint8, device="cuda")
    rows = []
    for N in (1, 8, 16, 32):
        idx = torch.empty((B, N, T), dtype=torch.int32, device="cuda")
        ln = torch.empty((B, N), dtype=torch.int32, device="cuda")
        sc = torch.empty((B, N), dtype=torch.float32, device="cuda")
        ts = event_ms(lambda: ctc_beam.launch(lib, x, B, T, CN, W, N, None, 0.0, 0.0, ws, idx, ln, sc, _lib.stream()), reps=20, warmup=2)
        rows.append(dict(nbest=N, beam_width=W, **spread(ts)))
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
    with_mbr = None
    if not plain_only:
        with_mbr = BatchedTFLiteModel(model, batch_size=B, max_frames=1024, beam_width=16, mbr_nbest=8)
        with_mbr.predict_indices(clips)
    t_plain, t_mbr = [], []
    for _ in range(4):                                    # alternated: 4 rounds of REPS / 2 replays each way
        t_plain += event_ms(lambda: plain._run(0, False), reps=REPS // 2, warmup=2)
        if with_mbr is not None:
            t_mbr += event_ms(lambda: with_mbr._run(0, False), reps=REPS // 2, warmup=2)
    res = dict(batch=B, beam_width=16, beam_top1_replay=spread(t_plain))
    if with_mbr is not None:
        res.update(mbr_nbest=8, mbr_replay=spread(t_mbr), added_ms_at_median=spread(t_mbr)["median_ms"] - spread(t_plain)["median_ms"])
    torch.cuda.synchronize()
    return res


def synthetic_accuracy():
    import torch
    from ishara_amd import mbr
    from ishara_amd.ctc import ctc_beam_nbest_device
    from ishara_amd.evaluation import levenshtein
    rows = []
    for noise in (1.5, 2.0, 2.5):
        x, phrases = noisy_logits(7, 256, 128, noise)
        hyp = ctc_beam_nbest_device(torch.from_numpy(x).cuda(), beam_width=32, nbest=16)
        idx, ln, best = mbr.mbr_select(*hyp, inv_temp=1.0, mode=1, C=CN)
        top = [hyp[0][b, 0, :max(int(hyp[1][b, 0]), 0)].tolist() for b in range(len(phrases))]
        idx, ln = idx.cpu().numpy(), ln.cpu().numpy()
        pick = [idx[b, :ln[b]].tolist() for b in range(len(phrases))]

        def score(decodes):
            return float(np.mean([(len(t) - levenshtein(d, t)) / len(t) for d, t in zip(decodes, phrases)]))
        rows.append(dict(noise=noise, clips=len(phrases), top1_score=score(top), mbr_score=score(pick), moved=int((best.cpu().numpy() > 0).sum())))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain-only", action="store_true", help="only the beam wrapper's replay (runs on a checkout without ishara_amd.mbr)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mbr_bench: no GPU: nothing here can be measured on the host")
    from ishara_amd.build import source_hash
    res = dict(workload=f"ishara_mbr_select at B {B}, T {T}, C {CN}, mode 1; BatchedTFLiteModel replay of a configs[1]-sized bf16 model at batch {B}, beam_width 16",
               source_hash=source_hash(), device=torch.cuda.get_device_name(0))
    if a.plain_only:
        res.update(replay=replays(True))
    else:
        res.update(select_alone=select_alone(), beam_alone=beam_alone(), replay=replays(False), synthetic_accuracy=synthetic_accuracy(),
                   note="event pairs around single launches / replays with the device idle before each.  synthetic_accuracy is SYNTHETIC: logits built "
                        "from random target phrases plus Gaussian noise, votes at temperature 1; no accuracy effect on real data is measured: there "
                        "is no dataset and there are no trained weights")
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
