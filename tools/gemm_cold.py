#!/usr/bin/env python3
"""Warm vs cold timing of the A-stationary NT GEMM and the transposed-read wgrad: the same launch over ONE buffer set (its 150 MB working
set stays in the 256 MB Infinity Cache between launches) against a rotation over NB distinct buffer sets (every launch reads and writes
memory the chip has not touched for NB-1 launches — what a launch sees inside the model).

    python tools/gemm_cold.py [--as-flags 51,115] [--nt-only] [--shape 98304,512,256]

--as-flags: ishara_debug_set_as_flags values to time the NT GEMMs under, one line each (51 the A-stationary kernels, 115 with the
C-stationary route for K = 512 -> N = 256: the decision gate of gemm_cs.hip; 371 = 115 | 256 keeps K = 768 -> N = 256 on the tile kernel:
`--nt-only --shape 98304,768,256 --as-flags 371,115` is that shape's gate); default: the library default alone."""
import argparse, ctypes as C, sys, torch
sys.path.insert(0, ".")
from ishara_amd import _lib
lib = _lib.load()
st = _lib.stream
ap = argparse.ArgumentParser()
ap.add_argument("--as-flags", default="-1")
ap.add_argument("--nt-only", action="store_true")
ap.add_argument("--shape", default="", help="M,K,N: this shape alone")
ap.add_argument("--repeats", type=int, default=3, help="cold repeats per line: the minimum and max - min are printed")
args = ap.parse_args()
FLAGS = [int(f) for f in args.as_flags.split(",")]
NB = 12
def timeit(fn, n):
    for i in range(min(n, NB)): fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n): fn(i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
SHAPES = [tuple(int(v) for v in args.shape.split(","))] if args.shape else [(98304, 256, 512), (98304, 512, 256), (98304, 256, 256), (98304, 256, 768)]
for (M, K, N) in SHAPES:
    xs = [torch.randn(M, K, device="cuda").bfloat16() for _ in range(NB)]
    ys = [torch.empty(M, N, device="cuda", dtype=torch.bfloat16) for _ in range(NB)]
    rs = [torch.randn(M, N, device="cuda").bfloat16() for _ in range(NB)]
    W = torch.randn(K, N, device="cuda") / K ** 0.5
    b = torch.randn(N, device="cuda")
    sc, scp = _lib.aligned(lib.ishara_op_scratch_bytes(M, K, N), "cuda")
    for flags in FLAGS:
        lib.ishara_debug_set_as_flags(flags)
        out = {}
        for name, resid, act in (("plain", False, 0), ("+resid", True, 0), ("+swish", False, 1)):
            f = lambda i, rot: lib.ishara_op_dense_fwd_ex(1, _lib.ptr(xs[i % NB if rot else 0]), _lib.ptr(W), _lib.ptr(b), _lib.ptr(rs[i % NB if rot else 0]) if resid else None,
                                                          _lib.ptr(ys[i % NB if rot else 0]), M, K, N, act, scp, st())
            w = min(timeit(lambda i: f(i, False), 24) for _ in range(3))
            cs = [timeit(lambda i: f(i, True), 24) for _ in range(args.repeats)]
            out[name] = (w, min(cs), max(cs) - min(cs))
        kern = lib.ishara_debug_dense_kernel_name(1, M, K, N, 0, 0).decode()
        print(f"NT  M{M} K{K} N{N} as_flags {flags} ({kern}): " + "  ".join(f"{k}: warm {w:.1f} cold {c:.1f} us (spread of {args.repeats} repeats {sp:.1f})" for k, (w, c, sp) in out.items()), flush=True)
    lib.ishara_debug_set_as_flags(-1)
    if args.nt_only:
        del xs, ys, rs
        continue
    dys = ys
    dW = torch.zeros(K, N, device="cuda"); db = torch.zeros(N, device="cuda")
    g = lambda i, rot: lib.ishara_op_dense_bwd(1, _lib.ptr(xs[i % NB if rot else 0]), _lib.ptr(W), _lib.ptr(dys[i % NB if rot else 0]), None, _lib.ptr(dW), _lib.ptr(db), M, K, N, scp, st())
    w = min(timeit(lambda i: g(i, False), 24) for _ in range(3))
    c = min(timeit(lambda i: g(i, True), 24) for _ in range(3))
    print(f"TN  M{M} K{K} N{N}: warm {w:.1f} cold {c:.1f} us (wgrad + slab sums + shadow build)", flush=True)
    del xs, ys, rs, dys
