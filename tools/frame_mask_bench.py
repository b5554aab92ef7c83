#!/usr/bin/env python3
"""What per-clip frame lengths cost (profiles/r11_frame_mask.json): one training step (forward, CTC, backward, optimizer) of the
benchmark's model — configs[1]: get_model(dim=256, 2 + 2 blocks), B 256, T 384, bf16, dropout on — in three variants that take turns:

  no_lengths      train_on_batch(x, y): the unmasked launches, what bench.py times
  lengths_all_T   frame_lengths = T for every clip: the same arithmetic through the lengths route (masked attention kernels with the
                  two-kernel backward, masked time means, no per-sample-affine weight gradient, two-kernel BatchNorm / depthwise backward);
                  its distance to no_lengths is the price of the less fused launches
  lengths_ragged  frame_lengths uniform in [T/4, T]: the key loops of the attention and the masked means stop at n_b

Timing (measuring-on-mi355x): device events around whole steps, after a warm-up of every variant; the variants take turns inside each
repeat, so drift hits them alike.  Nothing is flushed or rotated: the caches are in the state of a training run (a step moves several GiB,
far beyond the Infinity Cache).  Reported per variant: median, min, max (and the 10th / 90th percentile) over --reps repeats, in
milliseconds.  Nothing is gated.  Not measured here: per-kernel times (no profiler run), other shapes, f32.

    python tools/frame_mask_bench.py --out profiles/r11_frame_mask.json

Needs a GPU: without one it fails, there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(dim=256, num_conv_squeeze_blocks=2, num_conv_conform_blocks=2, kernel_sizes=[11, 5, 3], num_conv_per_block=3, dropout_rate=0.2,
          num_heads=8, expansion_factor=2, transformer_kernel_size=15, input_shape=(384, 224))


def _stats(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(p * len(v)))]
    return dict(median=q(0.5), min=v[0], p10=q(0.1), p90=q(0.9), max=v[-1])


def run(args):
    import numpy as np
    import torch
    from ishara_amd import get_model
    B = args.batch
    T, F = KW["input_shape"]
    model = get_model(**KW, dtype="bf16", max_batch=B, device="cuda:0", seed=0)
    model.optimizer.learning_rate = 1e-3
    g = np.random.default_rng(1)
    x = torch.from_numpy(g.standard_normal((B, T, F)).astype(np.float32)).cuda()
    y = np.full((B, 64), 59, np.int64)
    for b in range(B):
        n = int(g.integers(8, 32))
        y[b, :n] = g.integers(0, 59, n)
    y = torch.from_numpy(y).cuda()
    ragged = torch.from_numpy(g.integers(T // 4, T + 1, B).astype(np.int32)).cuda()
    variants = dict(no_lengths=None, lengths_all_T=torch.full((B,), T, dtype=torch.int32, device="cuda"), lengths_ragged=ragged)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def step(fl):
        torch.cuda.synchronize()
        e0.record()
        model.train_on_batch(x, y, frame_lengths=fl)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        for fl in variants.values():
            step(fl)
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fl in variants.items():
            times[k].append(step(fl))
    out = dict(workload=f"configs[1] training step, B={B} T={T} d=256 2+2 blocks bf16 dropout 0.2", reps=args.reps, warmup=args.warmup,
               mean_ragged_length=float(ragged.float().mean().item()), step_ms={k: _stats(v) for k, v in times.items()})
    med = lambda k: out["step_ms"][k]["median"]
    out["summary_ms"] = dict(lengths_all_T_minus_no_lengths=med("lengths_all_T") - med("no_lengths"),
                             lengths_ragged_minus_no_lengths=med("lengths_ragged") - med("no_lengths"),
                             lengths_ragged_minus_lengths_all_T=med("lengths_ragged") - med("lengths_all_T"))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bench", default=None, help="JSON file with bench.py results of this tree and the parent's, copied into the profile under 'bench_py'")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("frame_mask_bench: no GPU (nothing is measured without one)")
    from ishara_amd.build import source_hash
    res = dict(device=torch.cuda.get_device_name(0), source_hash=source_hash(),
               timing="device events around whole training steps, variants taking turns, warmed up; milliseconds; median and spread over the repeats",
               step=run(a))
    if a.bench:
        with open(a.bench) as f:
            res["bench_py"] = json.load(f)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
