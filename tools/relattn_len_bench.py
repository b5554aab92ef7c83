#!/usr/bin/env python3
"""What the Squeezeformer family's attention with per-clip lengths costs (profiles/r12_relattn_lengths.json).

Operator level, bf16, H 8, dh 64, B 8, at T 199 and T 99 (the attention shapes of a T0 = 800 clip), forward and backward timed apart:
  parent       ishara_op_relattn_fwd / _bwd: no lengths (a NULL key_len), the fp32 lane kernels of relattn_len.hip.  In r12_relattn_lengths.json
               this variant ran the lane kernels' earlier copies without the key_len argument; r13_relattn_one_lane_set.json compares the two
  len_full     ishara_relattn_len_fwd / _bwd with key_len = T, the plan's route (MFMA forward, length-aware lane backward)
  len_ragged   the same with lengths drawn uniformly in [T/2, T]
  lane_full    the same as len_full with route = 1: the length-aware lane kernels, forward too
Each entry point also runs the pos_proj GEMM (forward) or its weight gradient and the zero fills (backward), the same work in every variant, so
a difference between two variants is the difference of their attention kernels.
Encoder level: the training pass (forward + backward) of SqueezeformerEncoder at the reference's defaults (16 layers, d 512, 8 heads, T0 800,
B 8, bf16, dropout 0.1): plain, mask_padding with full lengths, mask_padding with ragged lengths in [T0/2, T0].

Timing (measuring-on-mi355x): device events around single calls after a warm-up of every variant; the variants take turns inside each repeat,
on the same device in the same process.  No buffer is rotated or flushed.  Reported per variant: the median and the spread (min, 10th and 90th
percentile, max) over --reps repeats, in microseconds.  Nothing is gated.

    python tools/relattn_len_bench.py --out profiles/r12_relattn_lengths.json

Needs a GPU: without one it fails, there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16 = 1
B, H, DH = 8, 8, 64


def _stats(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(p * len(v)))]
    return dict(median=q(0.5), min=v[0], p10=q(0.1), p90=q(0.9), max=v[-1])


def _timed(torch, e0, e1, run):
    torch.cuda.synchronize()
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def operator_run(lib, T, args):
    import torch
    from ishara_amd import _lib
    d, R = H * DH, 2 * T - 1
    g = torch.Generator(device="cuda").manual_seed(T)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    q, k, v, dO = (rn(B * T, d).bfloat16() for _ in range(4))
    pe, Wpos, u, vb = rn(R, d), rn(d, d) / d ** 0.5, 0.5 * rn(d), 0.5 * rn(d)
    o, dq, dk, dv = (torch.empty(B * T, d, dtype=torch.bfloat16, device="cuda") for _ in range(4))
    lse = torch.empty(B * H * T, device="cuda")
    du, dvb, dW, dp = torch.empty(d, device="cuda"), torch.empty(d, device="cuda"), torch.empty(d, d, device="cuda"), torch.empty(R, d, device="cuda")
    full = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ragged = torch.randint(T // 2, T + 1, (B,), device="cuda", generator=g).to(torch.int32)
    keep, sc = _lib.aligned(int(lib.ishara_relattn_len_scratch_bytes(B, H, T, DH)), "cuda")
    P, st = _lib.ptr, _lib.stream()
    tail = (B, H, T, DH, 7, 5, C.c_float(args.rate))

    def fwd(kl, route):
        if kl is None:
            return lambda: _lib.check(lib.ishara_op_relattn_fwd(BF16, P(q), P(k), P(v), P(pe), P(Wpos), P(u), P(vb), P(o), P(lse), *tail, sc, st), "fwd")
        return lambda: _lib.check(lib.ishara_relattn_len_fwd(BF16, P(q), P(k), P(v), P(pe), P(Wpos), P(u), P(vb), P(o), P(lse), *tail, P(kl), route, sc, st), "len_fwd")

    def bwd(kl, route):
        if kl is None:
            return lambda: _lib.check(lib.ishara_op_relattn_bwd(BF16, P(q), P(k), P(v), P(u), P(vb), P(o), P(dO), P(dq), P(dk), P(dv), P(du), P(dvb), P(dW), P(dp), *tail, sc, st), "bwd")
        return lambda: _lib.check(lib.ishara_relattn_len_bwd(BF16, P(q), P(k), P(v), P(u), P(vb), P(o), P(dO), P(dq), P(dk), P(dv), P(du), P(dvb), P(dW), P(dp), *tail,
                                                             P(kl), route, sc, st), "len_bwd")

    variants = dict(parent=(None, 0), len_full=(full, 0), len_ragged=(ragged, 0), lane_full=(full, 1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        for kl, route in variants.values():
            fwd(kl, route)(); bwd(kl, route)()
    times = {n: dict(fwd=[], bwd=[]) for n in variants}
    for _ in range(args.reps):
        for n, (kl, route) in variants.items():
            times[n]["fwd"].append(_timed(torch, e0, e1, fwd(kl, route)))
            times[n]["bwd"].append(_timed(torch, e0, e1, bwd(kl, route)))
    del keep
    out = dict(shape=f"B={B} H={H} T={T} dh={DH} bf16 dropout {args.rate:g}", ragged_key_len=ragged.tolist(), reps=args.reps, variants={})
    for n, (kl, route) in variants.items():
        masked = 0 if kl is None else 1
        names = ["relattn_len_fwd_kernel", "relattn_len_bwd_dq_kernel+relattn_len_bwd_dkv_kernel+relattn_len_bwd_dpos_kernel"] if route == 1 else \
            [lib.ishara_debug_relattn_kernel_name(BF16, bw, T, DH, masked).decode() for bw in (0, 1)]
        out["variants"][n] = dict(fwd_kernel=names[0], bwd_kernel=names[1], fwd_us=_stats(times[n]["fwd"]), bwd_us=_stats(times[n]["bwd"]))
    med = lambda n, w: out["variants"][n][w + "_us"]["median"]
    out["summary_us"] = {f"{n}_minus_parent": dict(fwd=med(n, "fwd") - med("parent", "fwd"), bwd=med(n, "bwd") - med("parent", "bwd")) for n in variants if n != "parent"}
    return out


def encoder_run(args):
    import torch
    from ishara_amd.squeezeformer import SqueezeformerEncoder
    T0, F = 800, 80
    enc = SqueezeformerEncoder(F, 512, 16, 7, 15, 8, 4, 2, args.rate, args.rate, args.rate, args.rate, 31, False, seq_len=T0, max_batch=B, dtype="bf16", seed=1).train()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, T0, F, device="cuda", generator=g)
    dy = torch.randn(B, enc.T_out, 512, device="cuda", generator=g)
    full = torch.full((B,), T0, dtype=torch.int32, device="cuda")
    ragged = torch.randint(T0 // 2, T0 + 1, (B,), device="cuda", generator=g).to(torch.int32)
    variants = dict(plain=None, mask_padding_full=full, mask_padding_ragged=ragged)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def step(il):
        enc._forward(x, True, seed=7, input_len=il)
        enc._backward(dy, input_len=il)

    for _ in range(2):
        for il in variants.values():
            step(il)
    times = {n: [] for n in variants}
    for _ in range(args.reps):
        for n, il in variants.items():
            times[n].append(_timed(torch, e0, e1, lambda: step(il)))
    out = dict(shape=f"SqueezeformerEncoder defaults: 16 layers, d 512, 8 heads, T0 {T0}, B {B}, bf16, dropout {args.rate:g}: forward + backward", reps=args.reps,
               ragged_input_len=ragged.tolist(), step_us={n: _stats(t) for n, t in times.items()})
    out["summary_us"] = {f"{n}_minus_plain": out["step_us"][n]["median"] - out["step_us"]["plain"]["median"] for n in variants if n != "plain"}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rate", type=float, default=0.1, help="dropout rate")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("relattn_len_bench: no GPU (nothing is measured without one)")
    from ishara_amd import _lib
    from ishara_amd.build import source_hash
    lib = _lib.load()
    res = dict(device=torch.cuda.get_device_name(0), source_hash=source_hash(),
               timing="device events around single calls, variants taking turns, warmed up; microseconds; median and spread over the repeats",
               operator=[operator_run(lib, T, a) for T in (199, 99)], encoder=encoder_run(a))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
