#!/usr/bin/env python3
"""What minimum-risk (MWER) training costs on the device (ishara_ctc_nbest_grad, ishara_mwer_weights, Optimizer(mwer_nbest=...)).
Records, not pass marks:

  * ishara_ctc_nbest_grad at B 64 and 256, T 384, C 60, hypotheses of 20 to 30 symbols in rows of width T, N = 4, 8, 16, max_len 32:
    HIP-event time around one call (two kernels; device idle before each; median, min, max, 10th and 90th percentile), with the bytes
    of its workspace;
  * beside it the emulation it replaces: ishara_ctc_loss_ex over the logits replicated N times with the coefficients as sample_scale,
    then the sum over N on the torch side, the replication and the allocations included, alternated with the kernel in rounds in one
    process; the bytes the emulation allocates (replicated logits, N gradient planes, the loss workspace); `kernel_wins` says whether the
    kernel's 90th percentile is below the emulation's 10th; a point whose emulation does not fit in memory is recorded as such;
  * ishara_mwer_weights at the same points, and the beam search at width 8 that feeds them;
  * train_on_batch of a configs[1]-sized bf16 model at batch 64 with mwer_nbest 0 (twice: the option's defaults, and an Optimizer that
    never heard of it), 4 and 8, alternated in rounds.  The parent commit's step is not part of this record.
An event pair around a launch of a few microseconds includes the launch floor.  No accuracy figure: there is no dataset and there are
no trained weights.

    python tools/mwer_bench.py --out profiles/r25_mwer.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, CN, MAX_LEN = 384, 60, 32
BS = (64, 256)
NS = (4, 8, 16)
ROUNDS = 4


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


def nbest(g, B, N):
    """hypotheses of 20 to 30 symbols without the blank: per clip one base string, every slot a copy with three symbols changed"""
    idx = np.full((B, N, T), -1, np.int32)
    ln = g.integers(20, 31, (B, N)).astype(np.int32)
    for b in range(B):
        base = g.integers(0, CN - 1, 32)
        for n in range(N):
            h = base.copy()
            h[g.integers(0, 32, 3)] = g.integers(0, CN - 1, 3)
            idx[b, n, :ln[b, n]] = h[:ln[b, n]]
    return idx, ln


def kernels(reps):
    import torch
    from ishara_amd import _lib, ctc, ctc_beam, mwer
    lib = _lib.load()
    g = np.random.default_rng(25)
    out = []
    for B in BS:
        x = torch.from_numpy((g.standard_normal((B, T, CN)) * 2).astype(np.float32)).cuda()
        tg = np.full((B, 32), 59, np.int32)
        for b in range(B):
            n = int(g.integers(20, 31))
            tg[b, :n] = g.integers(0, CN - 1, n)
        tg_d = torch.from_numpy(tg).cuda()
        for N in NS:
            idx, ln = nbest(g, B, N)
            d_idx, d_ln = torch.from_numpy(idx).cuda(), torch.from_numpy(ln).cuda()
            coef = torch.from_numpy(g.standard_normal((B, N)).astype(np.float32)).cuda()
            nbytes = mwer.workspace_bytes(lib, B, T, N, MAX_LEN)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            G = torch.empty((B, T, CN), dtype=torch.float32, device="cuda")

            def kernel():
                mwer.ctc_nbest_grad(x, d_idx, d_ln, coef, None, 1.0, out=G, max_len=MAX_LEN, workspace=ws)

            L = 32
            labels = torch.full((B * N, L), CN - 1, dtype=torch.int64, device="cuda")
            flat_idx, flat_ln = d_idx.reshape(B * N, T)[:, :L].to(torch.int64), d_ln.reshape(B * N)
            keep = torch.arange(L, device="cuda")[None, :] < flat_ln[:, None]
            labels = torch.where(keep, flat_idx, labels).contiguous()
            emu_bytes = B * N * T * CN * 4 * 2 + int(lib.ishara_ctc_workspace_bytes(B * N, T, L))
            fits = B * N <= 65535 and emu_bytes < 24e9

            def emulation():
                xr = x[:, None].expand(B, N, T, CN).reshape(B * N, T, CN).contiguous()
                grad = torch.empty_like(xr)
                nll = torch.empty(B * N, dtype=torch.float32, device="cuda")
                lws = torch.empty(int(lib.ishara_ctc_workspace_bytes(B * N, T, L)), dtype=torch.uint8, device="cuda")
                _lib.check(lib.ishara_ctc_loss_ex(_lib.ptr(xr), _lib.ptr(labels), B * N, T, CN, L, CN - 1, _lib.ptr(nll), _lib.ptr(grad), C.c_float(1.0),
                                                  _lib.ptr(lws), None, _lib.ptr(coef.reshape(-1)), 0, _lib.stream()), "ishara_ctc_loss_ex")
                return grad.reshape(B, N, T, CN).sum(1)

            tk, te = [], []
            for _ in range(ROUNDS):
                tk += event_ms(kernel, reps)
                if fits:
                    te += event_ms(emulation, reps)
            rec = dict(B=B, N=N, T=T, C=CN, max_len=MAX_LEN, kernel=spread(tk), kernel_workspace_bytes=int(nbytes), emulation_bytes=int(emu_bytes))
            if fits:
                rec["emulation"] = spread(te)
                rec["kernel_wins"] = bool(rec["kernel"]["p90_ms"] < rec["emulation"]["p10_ms"])
                err = (emulation() - G).abs().max().item()
                rec["max_abs_difference_to_the_emulation"] = float(err)
            else:
                rec["emulation"] = "not run: the replicated batch exceeds the loss kernel's launch or the memory budget of this tool"
            logp = torch.from_numpy((-np.abs(g.standard_normal((B, N))) * 4 - 30).astype(np.float32)).cuda()
            rec["mwer_weights"] = spread(event_ms(lambda: mwer.mwer_weights(d_idx, d_ln, logp, tg_d, 1.0, True), reps * ROUNDS))
            out.append(rec)
            print(json.dumps(rec), flush=True)
            del ws, G
            torch.cuda.empty_cache()
        beam = spread(event_ms(lambda: ctc.ctc_beam_nbest_device(x, None, 8, 8), reps))
        out.append(dict(B=B, beam_search_width_8_nbest_8=beam))
        print(json.dumps(out[-1]), flush=True)
    return out


def train_steps(reps):
    import torch
    from ishara_amd import Optimizer, get_model
    import bench
    kw = dict(bench.CONFIGS[2]["kw"])                        # configs[1], as bench.py builds it
    Bt = 64
    g = np.random.default_rng(26)
    models = {}
    for name, opt in (("no_option", None), ("mwer_nbest_0", dict(mwer_nbest=0)), ("mwer_nbest_4", dict(mwer_nbest=4)), ("mwer_nbest_8", dict(mwer_nbest=8))):
        m = get_model(dtype="bf16", max_batch=Bt, seed=3, **kw)
        if opt is not None:
            m.compile(optimizer=Optimizer(learning_rate=1e-3, **opt))
        models[name] = m
    m0 = models["no_option"]
    x = g.standard_normal((Bt, kw["input_shape"][0], kw["input_shape"][1])).astype(np.float32)
    y = np.full((Bt, m0._cfg.max_label_len), m0.C - 1, np.int64)
    for b in range(Bt):
        n = int(g.integers(10, 31))
        y[b, :n] = g.integers(0, m0.C - 1, n)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    ts = {k: [] for k in models}
    for _ in range(ROUNDS):
        for name, m in models.items():
            ts[name] += event_ms(lambda m=m: m.train_on_batch(xd, yd), reps, warmup=2)
    rec = {k: spread(v) for k, v in ts.items()}
    rec["config"] = dict({k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, batch=Bt, dtype="bf16")
    rec["stats_mwer_nbest_4"] = models["mwer_nbest_4"].mwer_stats()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_mwer.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    import torch
    t0 = time.time()
    res = dict(workload=f"ishara_ctc_nbest_grad beside the replicated-loss emulation, ishara_mwer_weights and the width-8 beam search at T {T}, C {CN}, "
                        f"hypotheses of 20..30 symbols in rows of width {T}, max_len {MAX_LEN}; train_on_batch with mwer_nbest 0 / 4 / 8",
               device=torch.cuda.get_device_name(0), rounds=ROUNDS, reps_per_round=a.reps, kernels=kernels(a.reps))
    if not a.skip_train:
        try:
            res["train_on_batch"] = train_steps(a.reps)
        except Exception as e:      # the kernel records above are kept
            res["train_on_batch"] = f"failed: {type(e).__name__}: {e}"
    res["seconds"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
