#!/usr/bin/env python3
"""What the exponential moving average of the weights costs a training step.  On bench.py's default workload (BASELINE configs[1]: B = 256,
T = 384, bf16, dropout on, synthetic data), in ONE process after a warm-up of every leg, alternating the legs round by round:

  (a) use_ema off                     the step bench.py times; the code path of the parent commit
  (b) use_ema on                      + weight_average behind the optimizer step (two launches: the update, the record)
  (c) use_ema on, overwrite every 100 + the second weight-shadow refresh behind it; one step in 100 also writes theta

and the kernel times of weight_average / weight_swap from the handle's profiler (events around each launch on the launch stream: launch gaps
included; weight_average is two launches in one bracket) with their algorithmic bytes (12 n, 16 n with an overwrite frequency; 16 n for the
swap) and the resulting TB/s, and the host-clock time of one `with model.averaged_weights(): pass` (two swaps and two weight-shadow
refreshes, ending in a device synchronise).

    python tools/ema_bench.py --out part1.json                   # one process: the three legs, --rounds rounds of --steps steps each
    python tools/ema_bench.py --merge part1.json part2.json part3.json --bench-parent p1.json p2.json p3.json \\
           --bench-this t1.json t2.json t3.json --out profiles/r18_ema.json

--merge records the spread of leg (a) over the processes next to the ms/step of `python bench.py` runs of the parent commit and of this
commit taken in the same GPU visit, alternating (each file: bench.py's JSON result line), and judges leg (a) against the parent's spread and
(b) - (a) against the weight_average kernel's own time.  No GPU is needed to merge."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {
    "a_off": dict(use_ema=False, ema_overwrite_frequency=None),
    "b_ema": dict(use_ema=True, ema_overwrite_frequency=None),
    "c_ema_overwrite100": dict(use_ema=True, ema_overwrite_frequency=100),
}


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
        raise SystemExit("ema_bench: needs the GPU (there is no CPU path and no estimate)")
    cfg = B.CONFIGS[2]
    Bt = cfg["batch"]
    T, F = cfg["kw"]["input_shape"]
    model = get_model(**cfg["kw"], dtype="bf16", max_batch=Bt, device="cuda:0", seed=0)
    model.optimizer.learning_rate = 1e-3
    model.optimizer.ema_momentum = 0.99
    g = np.random.default_rng(1)                       # bench.py's rank-0 batch
    x = torch.from_numpy(g.standard_normal((Bt, T, F)).astype(np.float32)).cuda()
    y = np.full((Bt, 64), 59, np.int64)
    for b in range(Bt):
        n = int(g.integers(8, 32))
        y[b, :n] = g.integers(0, 59, n)
    y = torch.from_numpy(y).cuda()

    def run(leg, steps):
        for k, v in LEGS[leg].items():
            setattr(model.optimizer, k, v)
        for _ in range(steps):
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

    def kernel(key, fn):
        recs = [_profiled(model, fn)[key] for _ in range(args.kernel_reps)]
        per = [r["ms"] / r["launches"] for r in recs]
        by = recs[0]["bytes"] / recs[0]["launches"]
        return dict(ms_per_call=_spread(per), launches_per_run=recs[0]["launches"], algorithmic_bytes_per_call=by, tb_per_s=by / (_median(per) * 1e-3) / 1e12)

    def swap_in_and_out():
        with model.averaged_weights():
            pass
    kern = {"weight_average": kernel("weight_average", lambda: run("b_ema", 1)),
            "weight_average_overwrite100": kernel("weight_average", lambda: run("c_ema_overwrite100", 1)),
            "weight_swap": kernel("weight_swap", swap_in_and_out)}
    ctx = []
    for _ in range(args.kernel_reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        swap_in_and_out()
        torch.cuda.synchronize()
        ctx.append((time.perf_counter() - t0) * 1e3)
    st = model.ema_state()
    for k, v in LEGS["a_off"].items():
        setattr(model.optimizer, k, v)
    return dict(workload=cfg["workload"] + f", B={Bt}, T={T}, bf16",
                source_hash=source_hash(), n_train=model.n_train,
                timing=f"host clock around {args.steps} steps ending in a device synchronise, legs alternating for {args.rounds} rounds in one process after "
                       f"{args.warmup} warm-up steps of every leg; kernels: the handle's profiler (events around each launch, launch gaps included), "
                       f"{args.kernel_reps} profiled runs; averaged_weights: host clock around one enter + exit ending in a device synchronise, "
                       f"the first 2 of {args.kernel_reps + 2} dropped",
                ms_per_step={leg: _spread(v) for leg, v in ms.items()}, kernels=kern, averaged_weights_enter_exit_ms=_spread(ctx[2:]), last_ema_state=st)


def merge(args):
    parts = [json.load(open(p)) for p in args.merge]
    hashes = {p["source_hash"] for p in parts}
    if len(hashes) != 1:
        raise SystemExit(f"the parts come from different builds: {sorted(hashes)}")

    def bench_ms(paths):
        out = []
        for p in paths or ():
            lines = [l for l in open(p).read().splitlines() if l.startswith("{")]
            out.append(json.loads(lines[-1])["ms_per_step"])
        return out
    out = dict(parts[0])
    legs = {leg: [p["ms_per_step"][leg]["median"] for p in parts] for leg in LEGS}
    out["ms_per_step"] = {leg: _spread(v) for leg, v in legs.items()}
    out["ms_per_step_rounds"] = {leg: [p["ms_per_step"][leg]["runs"] for p in parts] for leg in LEGS}
    out["kernels"] = [p["kernels"] for p in parts]
    out["averaged_weights_enter_exit_ms"] = _spread([p["averaged_weights_enter_exit_ms"]["median"] for p in parts])
    out["timing"] = parts[0]["timing"] + f"; {len(parts)} processes, alternating with `python bench.py` runs of the parent commit and of this commit in the same GPU visit"
    parent, this = bench_ms(args.bench_parent), bench_ms(args.bench_this)
    a = out["ms_per_step"]["a_off"]
    judge = {}
    if parent:
        ps = _spread(parent)
        out["bench_py_parent_ms_per_step"] = ps
        tol = max(ps["spread"], a["spread"])
        judge["leg_a_vs_parent"] = dict(leg_a_median=a["median"], parent_min=ps["min"], parent_max=ps["max"], parent_spread=ps["spread"],
                                        inside_parent_spread=bool(ps["min"] - tol <= a["median"] <= ps["max"] + tol),
                                        rule="leg (a)'s median within [parent min, parent max] widened by the larger of the two spreads")
    else:
        out["bench_py_parent_ms_per_step"] = "not measured"
    out["bench_py_this_ms_per_step"] = _spread(this) if this else "not measured"
    # the off leg's run-to-run spread: over the processes, and over the rounds inside each process, whichever is larger
    a_spread = max([a["spread"]] + [p["ms_per_step"]["a_off"]["spread"] for p in parts])
    for leg, key, name in (("b_ema", "weight_average", "ema_cost"), ("c_ema_overwrite100", "weight_average_overwrite100", "ema_overwrite100_cost")):
        k = _median([p["kernels"][key]["ms_per_call"]["median"] for p in parts])
        delta = out["ms_per_step"][leg]["median"] - a["median"]
        judge[name] = dict(leg_minus_a_ms=delta, weight_average_kernel_ms=k, spread_of_leg_a_ms=a_spread,
                           exceeds_kernel_by_more_than_spread=bool(delta - k > a_spread))
    judge["ema_cost"]["rule"] = "the step-time increase with use_ema on must not exceed the kernel's own time by more than the run-to-run spread of the off leg"
    judge["ema_overwrite100_cost"]["note"] = "leg (c) also runs a second weight-shadow refresh per step, which the kernel time does not hold"
    out["judgement"] = judge
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--merge", nargs="+", default=None, help="part files of earlier runs of this tool (no GPU)")
    ap.add_argument("--bench-parent", nargs="*", default=None, help="bench.py result lines of the parent commit, same GPU visit")
    ap.add_argument("--bench-this", nargs="*", default=None, help="bench.py result lines of this commit, same GPU visit")
    a = ap.parse_args()
    res = merge(a) if a.merge else bench(a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
