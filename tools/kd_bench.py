#!/usr/bin/env python3
"""What knowledge distillation costs on the device (ishara_kd_grad, Optimizer(kd_weight=...), Model.set_teacher).  Records, not pass marks:

  (a) ishara_kd_grad at B 64 and 256, T 384, C 60, accumulate 1 (the training step's form), in four forms: with and without dlb, with and
      without kl_frame + kl_clip (the second form of each pair hands NULL): HIP-event time around one call (device idle before each;
      median, min, max, 10th and 90th percentile), with the bytes the call moves.  Beside it the emulation it replaces, in torch:
      log_softmax / softmax / kl_div under autograd for the gradient, the add into dlogits, and the repack of the sum into the padded bf16
      rows; alternated with the kernel in rounds in one process.  `kernel_faster` says whether the kernel's 90th percentile is below the
      emulation's 10th; otherwise the record says not faster.
  (b) train_on_batch of a configs[1]-sized bf16 model at batch 64: the option off, on with a same-size teacher attached (its forward runs
      inside the step), and on with teacher_logits= (an offline-cached teacher), alternated in rounds.  With --parent-root DIR (a built
      checkout of the parent commit) the off leg is also run from that tree, in a child process before and after the legs of this tree,
      and `off_path_unmoved` says whether the two off medians lie within each other's 10th-90th spread.
An event pair around a launch of a few microseconds includes the launch floor.  No accuracy figure: there is no dataset and there are
no trained weights.

    python tools/kd_bench.py --out profiles/r26_kd.json [--parent-root DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, CN = 384, 60
BS = (64, 256)
ROUNDS = 4
TAU = 2.0


def spread(ts):
    ts = np.sort(np.asarray(ts, np.float64))
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts[0]), max_ms=float(ts[-1]), p10_ms=float(np.percentile(ts, 10)),
                p90_ms=float(np.percentile(ts, 90)), reps=int(ts.size))


def event_ms(fn, reps, warmup=2):
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


def operator(reps):
    import torch
    import torch.nn.functional as F
    from ishara_amd import kd
    g = np.random.default_rng(26)
    out = []
    for B in BS:
        x = torch.from_numpy((g.standard_normal((B, T, CN)) * 2).astype(np.float32)).cuda()
        u = torch.from_numpy((g.standard_normal((B, T, CN)) * 2).astype(np.float32)).cuda()
        base = torch.from_numpy((g.standard_normal((B, T, CN)) * 0.01).astype(np.float32)).cuda()
        gs = 0.5 * TAU / B
        for want_dlb in (True, False):
            for want_kl in (True, False):
                dl = base.clone()
                dlb = torch.empty((B * T, 64), dtype=torch.int32, device="cuda") if want_dlb else None

                def kernel():
                    kd.kd_grad(x, u, None, 1.0 / TAU, "mean", gs, out=dl, accumulate=True, dlb=dlb, return_kl=want_kl)

                dl2 = base.clone()
                pad = torch.zeros((B * T, 128), dtype=torch.bfloat16, device="cuda") if want_dlb else None

                def emulation():
                    z = x.detach().requires_grad_(True)
                    kl = F.kl_div(F.log_softmax(z * (1.0 / TAU), -1), F.softmax(u * (1.0 / TAU), -1), reduction="none").sum(-1)      # [B, T]
                    clip = kl.mean(1)
                    (clip.sum() * (gs * TAU)).backward()
                    dl2.add_(z.grad)
                    if want_dlb:
                        pad[:, :CN] = dl2.reshape(B * T, CN).to(torch.bfloat16)
                    return clip if want_kl else None

                tk, te = [], []
                for _ in range(ROUNDS):
                    tk += event_ms(kernel, reps)
                    te += event_ms(emulation, reps)
                moved = B * T * CN * 4 * 4 + (B * T * 256 if want_dlb else 0) + (B * T * 4 * 2 + B * 4 if want_kl else 0)
                rec = dict(B=B, T=T, C=CN, accumulate=1, dlb=want_dlb, kl=want_kl, bytes_moved=int(moved), kernel=spread(tk), emulation=spread(te))
                rec["kernel_gb_per_s_at_median"] = moved / (rec["kernel"]["median_ms"] * 1e-3) / 1e9
                rec["kernel_faster"] = bool(rec["kernel"]["p90_ms"] < rec["emulation"]["p10_ms"])
                # one more call of each from the same start, to compare what they compute
                dl.copy_(base); dl2.copy_(base)
                kernel(); emulation()
                rec["max_abs_difference_to_the_emulation"] = float((dl - dl2).abs().max().item())
                out.append(rec)
                print(json.dumps(rec), flush=True)
    return out


def _train_setup(kw, Bt):
    import torch
    g = np.random.default_rng(27)
    x = g.standard_normal((Bt, kw["input_shape"][0], kw["input_shape"][1])).astype(np.float32)
    y = np.full((Bt, 64), 59, np.int64)
    for b in range(Bt):
        n = int(g.integers(10, 31))
        y[b, :n] = g.integers(0, 59, n)
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def off_leg(reps, rounds=ROUNDS):
    """train_on_batch with an Optimizer at its defaults, from whichever tree is first on sys.path"""
    import bench
    from ishara_amd import get_model
    kw = dict(bench.CONFIGS[2]["kw"])                        # configs[1], as bench.py builds it
    m = get_model(dtype="bf16", max_batch=64, seed=3, **kw)
    xd, yd = _train_setup(kw, 64)
    ts = []
    for _ in range(rounds):
        ts += event_ms(lambda: m.train_on_batch(xd, yd), reps, warmup=2)
    return spread(ts)


def parent_off_leg(parent_root, reps):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-leg-only", "--root", parent_root, "--reps", str(reps)], capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        return f"failed: {r.stderr[-400:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


def train_steps(reps, parent_root):
    import torch
    import bench
    from ishara_amd import Optimizer, get_model
    kw = dict(bench.CONFIGS[2]["kw"])
    Bt = 64
    rec = {}
    if parent_root:
        rec["off_parent_before"] = parent_off_leg(parent_root, reps)
    models = {}
    for name in ("off", "on_teacher_model", "on_teacher_logits"):
        m = get_model(dtype="bf16", max_batch=Bt, seed=3, **kw)
        if name != "off":
            m.compile(optimizer=Optimizer(learning_rate=1e-3, kd_weight=0.5, kd_temperature=TAU))
        models[name] = m
    teacher = get_model(dtype="bf16", max_batch=Bt, seed=5, **kw)
    models["on_teacher_model"].set_teacher(teacher)
    xd, yd = _train_setup(kw, Bt)
    rows = teacher(xd, training=False).clone()
    calls = dict(off=lambda m: m.train_on_batch(xd, yd), on_teacher_model=lambda m: m.train_on_batch(xd, yd),
                 on_teacher_logits=lambda m: m.train_on_batch(xd, yd, teacher_logits=rows))
    ts = {k: [] for k in models}
    for _ in range(ROUNDS):
        for name, m in models.items():
            ts[name] += event_ms(lambda m=m, f=calls[name]: f(m), reps, warmup=2)
    rec.update({k: spread(v) for k, v in ts.items()})
    rec["teacher_forward"] = spread(event_ms(lambda: teacher(xd, training=False), reps * ROUNDS))
    rec["config"] = dict({k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, batch=Bt, dtype="bf16", kd_weight=0.5, kd_temperature=TAU)
    rec["stats_on_teacher_logits"] = models["on_teacher_logits"].kd_stats()
    if parent_root:
        rec["off_parent_after"] = parent_off_leg(parent_root, reps)
        legs = [v for v in (rec["off_parent_before"], rec["off_parent_after"]) if isinstance(v, dict)]
        if legs:
            par = dict(median_ms=float(np.median([v["median_ms"] for v in legs])), p10_ms=min(v["p10_ms"] for v in legs), p90_ms=max(v["p90_ms"] for v in legs))
            off = rec["off"]
            rec["off_parent"] = par
            rec["off_path_unmoved"] = bool(par["p10_ms"] <= off["median_ms"] <= par["p90_ms"] and off["p10_ms"] <= par["median_ms"] <= off["p90_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE_ROOT, "profiles", "r26_kd.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its off leg is run in a child process")
    ap.add_argument("--root", default=HERE_ROOT, help="the tree to import ishara_amd and bench from")
    ap.add_argument("--off-leg-only", action="store_true", help="print the off leg of --root as one JSON line and exit")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if a.off_leg_only:
        print(json.dumps(off_leg(a.reps)))
        return
    t0 = time.time()
    res = dict(workload=f"ishara_kd_grad (accumulate 1) beside the torch emulation at T {T}, C {CN}, B {list(BS)}; train_on_batch of configs[1] bf16 at batch 64 with "
                        "distillation off / on with a same-size teacher / on with teacher_logits",
               device=torch.cuda.get_device_name(0), rounds=ROUNDS, reps_per_round=a.reps, operator=operator(a.reps))
    if not a.skip_train:
        try:
            res["train_on_batch"] = train_steps(a.reps, a.parent_root)
        except Exception as e:      # the operator records above are kept
            res["train_on_batch"] = f"failed: {type(e).__name__}: {e}"
    res["accuracy"] = "not measured: there is no dataset and there are no trained weights"
    res["seconds"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
