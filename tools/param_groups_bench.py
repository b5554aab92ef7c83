#!/usr/bin/env python3
"""What the optimizer's parameter groups cost.  At the parameter count and on the real entry table of bench.py's default workload (BASELINE
configs[1]: B = 256, T = 384, bf16, dropout on, synthetic data), in ONE process, the legs alternating round by round after a warm-up:

Kernels (the model-free operator entry points on buffers of n_train elements, step number 6: rectified, no Lookahead sync; device events
around a burst of calls, so launch gaps are inside the figure):
  plain_ex        ishara_optimizer_op_step with a record: the existing radam_lookahead_ex launch, the baseline
  groups_default  ishara_optimizer_op_step_groups, every row (1, 1, 0): the chunk-table launch and the grouped pass
  groups_half     the same with whole tensors frozen until about half of the bytes are
  mask            ishara_gradient_mask_groups on the half-frozen rows
  empty_launch    ishara_optimizer_op_step on one element: the floor of one launch
Whole step (host clock around a burst of train_on_batch ending in a device synchronise):
  off             param_groups None, apply_weight_decay on
  no_decay        param_groups = train_state.no_decay_groups(entries), otherwise the same
and, from the handle's profiler, the update's own launch bracket inside such a step for both (update_in_step: the buffers come from HBM
there, while a burst of operator calls on 212 MB finds them in the 256 MB last-level cache).

    python tools/param_groups_bench.py --out profiles/r22_param_groups.json [--parent-json FILE]
    python tools/param_groups_bench.py --whole-step-off-only --out FILE        # runs on a checkout without the feature (the parent commit)

The expectation the judgement checks: groups_default moves the same 28 n bytes as plain_ex plus a table that stays in L2, so its median
should lie within plain_ex's 10th-90th percentile spread plus empty_launch (the chunk table is a launch of its own); groups_half should
take correspondingly less.  Where that does not hold the gap is in the output, not hidden.  Nothing here is asserted by a test."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_LEGS = ("plain_ex", "groups_default", "groups_half", "mask", "empty_launch")
STEP_LEGS = ("off", "no_decay")
LR, WD, ITERATION = 1e-3, 1e-4, 6


def _pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def _spread(v):
    return dict(runs=[round(x, 5) for x in v], min=min(v), p10=_pct(v, 0.1), median=_pct(v, 0.5), p90=_pct(v, 0.9), max=max(v))


def _workload(root):
    sys.path.insert(0, root)
    import torch
    import bench as B
    from ishara_amd import get_model
    if not torch.cuda.is_available():
        raise SystemExit("param_groups_bench: needs the GPU (there is no CPU path and no estimate)")
    cfg = B.CONFIGS[2]
    Bt = cfg["batch"]
    T, F = cfg["kw"]["input_shape"]
    model = get_model(**cfg["kw"], dtype="bf16", max_batch=Bt, device="cuda:0", seed=0)
    model.optimizer.learning_rate, model.optimizer.weight_decay, model.optimizer.apply_weight_decay = LR, WD, True
    g = np.random.default_rng(1)                       # bench.py's rank-0 batch
    x = torch.from_numpy(g.standard_normal((Bt, T, F)).astype(np.float32)).cuda()
    y = np.full((Bt, 64), 59, np.int64)
    for b in range(Bt):
        n = int(g.integers(8, 32))
        y[b, :n] = g.integers(0, 59, n)
    return cfg, model, x, torch.from_numpy(y).cuda()


def _whole_step(model, x, y, legs, args, groups_of):
    import torch

    def run(leg, steps):
        if "no_decay" in legs:
            model.optimizer.param_groups = groups_of(leg)
        for _ in range(steps):
            model.train_on_batch(x, y)

    for leg in legs:
        run(leg, args.warmup)
    ms = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            run(leg, 1)                                # the switch of the option (resolving the patterns, the 16 S byte upload) is not the step's cost
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(leg, args.steps)
            torch.cuda.synchronize()
            ms[leg].append((time.perf_counter() - t0) / args.steps * 1e3)
    return {leg: _spread(v) for leg, v in ms.items()}


def _in_step(model, x, y, no_decay, args):
    """the update's own launch bracket inside a training step (the handle's profiler: events around the launches, launch gaps included)"""
    out = {}
    for leg, key in (("off", "radam_lookahead"), ("no_decay", "radam_lookahead_groups")):
        model.optimizer.param_groups = no_decay if leg == "no_decay" else None
        recs = [model.profile_step(x, y) for _ in range(args.kernel_rounds)]
        out[leg] = dict(key=key, ms_per_call=_spread([r[key]["ms"] / r[key]["launches"] for r in recs]))
    model.optimizer.param_groups = None
    return out


def _kernels(model, args):
    import torch
    from ishara_amd import _lib, train_state as TS
    lib, n, F32 = model._lib, model.n_train, C.c_float
    seg, rows = TS.param_group_rows(model.entries, n, [{"match": "*"}])
    S = len(rows)
    half = rows.copy()
    frozen = 0
    for s in np.argsort(-np.diff(seg)):                # whole tensors, the largest first, until half of the elements are frozen
        if frozen + int(seg[s + 1] - seg[s]) <= n // 2:
            half[s]["frozen"] = 1
            frozen += int(seg[s + 1] - seg[s])
    dev = model.device
    r = np.random.default_rng(2)
    bufs = [torch.from_numpy(a.astype(np.float32)).to(dev) for a in (0.5 * r.standard_normal(n), 1e-2 * r.standard_normal(n), np.zeros(n), np.zeros(n))]
    theta, grad, m, v = bufs
    slow = theta.clone()
    rec = torch.zeros(4, dtype=torch.int32, device=dev)
    rec[1] = int(np.array([0.75], np.float32).view(np.int32)[0])
    seg_d = torch.from_numpy(seg).to(dev)
    rows_d = {k: torch.from_numpy(a.view(np.int32).copy()).to(dev) for k, a in (("default", rows), ("half", half))}
    ws = torch.empty(int(lib.ishara_param_groups_workspace_bytes(n, S)), dtype=torch.uint8, device=dev)
    head = lambda cnt: (_lib.ptr(theta), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), _lib.ptr(slow), cnt, ITERATION, F32(LR), F32(WD), _lib.ptr(rec), 1)      # noqa: E731
    grouped = lambda key: lib.ishara_optimizer_op_step_groups(*head(n), _lib.ptr(seg_d), _lib.ptr(rows_d[key]), S, _lib.ptr(ws), _lib.stream())      # noqa: E731
    calls = dict(plain_ex=lambda: lib.ishara_optimizer_op_step(*head(n), _lib.stream()),
                 groups_default=lambda: grouped("default"), groups_half=lambda: grouped("half"),
                 mask=lambda: lib.ishara_gradient_mask_groups(None, _lib.ptr(grad), n, _lib.ptr(seg_d), _lib.ptr(rows_d["half"]), S, _lib.ptr(ws), _lib.stream()),
                 empty_launch=lambda: lib.ishara_optimizer_op_step(*head(1), _lib.stream()))
    for leg in KERNEL_LEGS:
        for _ in range(args.kernel_burst):
            _lib.check(calls[leg](), leg)
    torch.cuda.synchronize()
    ms = {leg: [] for leg in KERNEL_LEGS}
    for _ in range(args.kernel_rounds):
        for leg in KERNEL_LEGS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.kernel_burst):
                calls[leg]()
            e1.record()
            e1.synchronize()
            ms[leg].append(e0.elapsed_time(e1) / args.kernel_burst)
    out = {leg: dict(ms_per_call=_spread(v)) for leg, v in ms.items()}
    live = n - frozen
    for leg, by in (("plain_ex", 28.0 * n), ("groups_default", 28.0 * n), ("groups_half", 28.0 * live), ("mask", 4.0 * frozen)):
        out[leg].update(algorithmic_bytes=by, tb_per_s=by / (out[leg]["ms_per_call"]["median"] * 1e-3) / 1e12)
    return out, dict(segments=S, frozen_elements=frozen, frozen_share=frozen / n)


def bench(args):
    cfg, model, x, y = _workload(args.root)
    Bt = cfg["batch"]
    T, _ = cfg["kw"]["input_shape"]
    timing = (f"whole step: host clock around {args.steps} steps ending in a device synchronise, legs alternating for {args.rounds} rounds in one process "
              f"after {args.warmup} warm-up steps of every leg, one untimed step behind every switch of leg")
    base = dict(workload=cfg["workload"] + f", B={Bt}, T={T}, bf16", n_train=model.n_train)
    if args.whole_step_off_only:
        return dict(base, timing=timing, ms_per_step=_whole_step(model, x, y, ("off",), args, None))
    from ishara_amd import train_state as TS
    from ishara_amd.build import source_hash
    no_decay = TS.no_decay_groups(model.entries)
    steps = _whole_step(model, x, y, STEP_LEGS, args, lambda leg: no_decay if leg == "no_decay" else None)
    in_step = _in_step(model, x, y, no_decay, args)
    kern, table = _kernels(model, args)
    k = {leg: kern[leg]["ms_per_call"] for leg in KERNEL_LEGS}
    allowance = k["plain_ex"]["p90"] - k["plain_ex"]["p10"] + k["empty_launch"]["median"]
    gap = k["groups_default"]["median"] - k["plain_ex"]["median"]
    judgement = dict(default_minus_plain_ms=gap, allowance_ms=allowance, default_within_allowance=bool(gap <= allowance),
                     half_over_default=k["groups_half"]["median"] / k["groups_default"]["median"],
                     half_frozen_takes_less=bool(k["groups_half"]["median"] < k["groups_default"]["median"]),
                     no_decay_minus_off_ms=steps["no_decay"]["median"] - steps["off"]["median"],
                     in_step_update_no_decay_minus_off_ms=in_step["no_decay"]["ms_per_call"]["median"] - in_step["off"]["ms_per_call"]["median"],
                     spread_of_off_ms=steps["off"]["max"] - steps["off"]["min"],
                     rule="groups_default - plain_ex (medians) against plain_ex's p90 - p10 plus one empty launch; groups_half against groups_default; "
                          "the whole step with no_decay_groups against the step without groups and the spread of the latter")
    out = dict(base, source_hash=source_hash(), **table,
               timing=timing + f"; kernels: device events around {args.kernel_burst} calls, legs alternating for {args.kernel_rounds} rounds, step number "
                      f"{ITERATION}, a record with coef 0.75 and the skip switch on",
               ms_per_step=steps, update_in_step=in_step, kernels=kern, judgement=judgement)
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        out["parent_commit"] = dict(ms_per_step=parent["ms_per_step"], note="the plain step of the parent commit, its own build, measured in the same visit")
        judgement["off_minus_parent_off_ms"] = steps["off"]["median"] - parent["ms_per_step"]["off"]["median"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=ROOT, help="the checkout whose ishara_amd and bench are measured")
    ap.add_argument("--whole-step-off-only", action="store_true")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-burst", type=int, default=20)
    ap.add_argument("--kernel-rounds", type=int, default=15)
    a = ap.parse_args()
    res = bench(a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
