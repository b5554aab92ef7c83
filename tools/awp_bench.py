#!/usr/bin/env python3
"""What adversarial weight perturbation costs a training step.  On bench.py's default workload (BASELINE configs[1]: B = 256, T = 384, bf16,
dropout on, synthetic data), in ONE process after a warm-up of every leg, alternating the legs round by round:

  (a) awp_delta None        the step bench.py times; the code path of the parent commit
  (b) awp_delta 0.2         pass 1, ishara_awp_perturb, weight shadows, pass 2, ishara_awp_restore, the optimizer step
  (c) two plain passes      loss_and_gradients twice on the same seed, then the optimizer step: what (b) costs without its new launches

and the per-launch times of awp_norms (four launches in one bracket), awp_perturb, awp_restore and of the weight-shadow refresh (the launch
ishara_sync_weights makes; timed where the optimizer step brackets it, key weight_shadows) from the handle's profiler (events around each
launch on the launch stream: launch gaps included), with their algorithmic bytes (4 n, 16 n, 8 n) and the resulting TB/s.

    python tools/awp_bench.py --out profiles/r19_awp.json

The judgement compares (b) - (c), the cost beyond two forward + backward passes, with the sum of the new launches' own times and with the
run-to-run spread of leg (a); (b) / (a) is reported next to it.  Nothing here is asserted by a test."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("a_off", "b_awp", "c_two_passes")
DELTA = 0.2


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _spread(v):
    return dict(runs=[round(x, 4) for x in v], min=min(v), median=_median(v), max=max(v), spread=max(v) - min(v))


def _profiled(model, fn):
    """fn() with the handle's profiler on -> {key: {launches, ms, bytes}}"""
    from ishara_amd import _lib
    _lib.check(model._lib.ishara_profile_enable(model._h, 1))
    try:
        fn()
        buf = C.create_string_buffer(1 << 16)
        n = model._lib.ishara_profile_report(model._h, buf, len(buf))
        if n < 0:
            _lib.check(n, "ishara_profile_report")
    finally:
        model._lib.ishara_profile_enable(model._h, 0)
    out = {}
    for line in buf.value.decode().splitlines():
        k, cnt, ms, by, _ = line.split()
        out[k] = dict(launches=int(cnt), ms=float(ms), bytes=float(by))
    return out


def bench(args):
    import torch
    import bench as B
    from ishara_amd import get_model
    from ishara_amd.build import source_hash
    if not torch.cuda.is_available():
        raise SystemExit("awp_bench: needs the GPU (there is no CPU path and no estimate)")
    cfg = B.CONFIGS[2]
    Bt = cfg["batch"]
    T, F = cfg["kw"]["input_shape"]
    model = get_model(**cfg["kw"], dtype="bf16", max_batch=Bt, device="cuda:0", seed=0)
    model.optimizer.learning_rate = 1e-3
    g = np.random.default_rng(1)                       # bench.py's rank-0 batch
    x = torch.from_numpy(g.standard_normal((Bt, T, F)).astype(np.float32)).cuda()
    y = np.full((Bt, 64), 59, np.int64)
    for b in range(Bt):
        n = int(g.integers(8, 32))
        y[b, :n] = g.integers(0, 59, n)
    y = torch.from_numpy(y).cuda()

    def run(leg, steps):
        model.optimizer.awp_delta = DELTA if leg == "b_awp" else None
        for _ in range(steps):
            if leg == "c_two_passes":
                seed = (model._step_seed + 0x9E3779B1 * model._steps) & 0xFFFFFFFF
                model.loss_and_gradients(x, y, seed=seed)
                model.loss_and_gradients(x, y, seed=seed)
                model.apply_gradients()
            else:
                model.train_on_batch(x, y)

    for leg in LEGS:
        run(leg, args.warmup)
    torch.cuda.synchronize()
    ms = {leg: [] for leg in LEGS}
    for _ in range(args.rounds):
        for leg in LEGS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(leg, args.steps)
            torch.cuda.synchronize()
            ms[leg].append((time.perf_counter() - t0) / args.steps * 1e3)

    recs = [_profiled(model, lambda: run("b_awp", 1)) for _ in range(args.kernel_reps)]
    kern = {}
    for key in ("awp_norms", "awp_perturb", "awp_restore", "weight_shadows"):
        per = [r[key]["ms"] / r[key]["launches"] for r in recs]
        by = recs[0][key]["bytes"] / recs[0][key]["launches"]
        kern[key] = dict(ms_per_call=_spread(per), calls_per_step=recs[0][key]["launches"], algorithmic_bytes_per_call=by,
                         tb_per_s=by / (_median(per) * 1e-3) / 1e12 if by else None)
    stats = model.awp_stats()
    model.optimizer.awp_delta = None

    a, b, c = (_spread(ms[leg]) for leg in LEGS)
    new_launches = sum(kern[k]["ms_per_call"]["median"] for k in ("awp_norms", "awp_perturb", "awp_restore")) + kern["weight_shadows"]["ms_per_call"]["median"]
    judgement = dict(awp_over_off=b["median"] / a["median"],
                     beyond_two_passes_ms=b["median"] - c["median"],
                     new_launches_ms=new_launches,
                     new_launches_share_of_awp_step=new_launches / b["median"],
                     spread_of_leg_a_ms=a["spread"],
                     beyond_two_passes_exceeds_new_launches_by_more_than_spread=bool(b["median"] - c["median"] - new_launches > a["spread"]),
                     rule="(b) - (c), the cost beyond two forward + backward passes and one optimizer step, against the new launches' own times "
                          "(norms, perturb, restore and one more weight-shadow refresh) and the run-to-run spread of leg (a)")
    return dict(workload=cfg["workload"] + f", B={Bt}, T={T}, bf16", source_hash=source_hash(), n_train=model.n_train,
                segments=model._awp["S"], awp_delta=DELTA,
                timing=f"host clock around {args.steps} steps ending in a device synchronise, legs alternating for {args.rounds} rounds in one process after "
                       f"{args.warmup} warm-up steps of every leg; kernels: the handle's profiler (events around each launch, launch gaps included), "
                       f"{args.kernel_reps} profiled steps of leg (b)",
                ms_per_step=dict(zip(LEGS, (a, b, c))), kernels=kern, judgement=judgement, last_awp_stats=stats)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=5)
    a = ap.parse_args()
    res = bench(a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
