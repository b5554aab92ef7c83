#!/usr/bin/env python3
"""What per-sample frame counts cost (profiles/r9_ctc_lengths.json).  Three measurements, all with device events around a block of
back-to-back launches after a warm-up, the median over --reps blocks (a block is sized so that every timed window is a few milliseconds
and every series a few tenths of a second):

  (a) the fixed-T loss must not have changed: ishara_ctc_loss at the benchmark's shape (B 256, T 384, L 64, C 60, with dlogits) from this
      build and from a second library built from the parent commit's csrc (--parent-lib), the two alternating block by block in one
      process.  The parent library is also loaded a second time from a copy of the file and timed against itself in the same loop (A/A):
      that difference is the noise floor of the comparison.  Accepted when new <= parent + |A/A difference|.
  (b) ragged batches: each *_ex entry point with lengths all T and with lengths uniform in [T/4, T] (informational);
  (c) ishara_amd.ctc_loss forward + backward against torch.nn.functional.ctc_loss on the same device tensors, at (B 16, T 200, C 60,
      S 32) and at the shape of (a) (informational: the path it replaces).

    python tools/ctc_lengths_bench.py --parent-lib PATH/libishara_hip.so --out profiles/r9_ctc_lengths.json

Needs a GPU: without one it fails, there is no fallback.  Until it has run on an MI355X the profile reads "not measured"."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, CN, L = 256, 384, 60, 64
SMALL = dict(B=16, T=200, C=60, S=32)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _series(runs, block, reps):
    """runs: name -> closure.  Every rep times one block of each closure, in turn -> name -> median ms per launch."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for run in runs.values():
        for _ in range(block):
            run()
    ts = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(block):
                run()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / block)
    return {k: _median(v) for k, v in ts.items()}


def _inputs(b, t, c, l, seed=0):
    g = np.random.default_rng(seed)
    x = (3.0 * g.standard_normal((b, t, c))).astype(np.float32)
    y = np.full((b, l), c - 1, np.int64)
    for i in range(b):
        n = int(g.integers(l // 8, l // 2 + 1))                      # fits T / 4 frames with room for repeats
        y[i, :n] = g.integers(0, c - 1, n)
    return x, y, g.integers(t // 4, t + 1, b).astype(np.int32)


def _foreign(path):
    """a second libishara_hip.so with the signatures this tool calls"""
    from ishara_amd import _lib
    lib = C.CDLL(path)
    for name in ("ishara_ctc_loss", "ishara_ctc_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def fixed_t(args):
    import torch
    from ishara_amd import _lib
    x, y, _ = _inputs(B, T, CN, L)
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tmp = tempfile.mkdtemp()
    copy = shutil.copy(args.parent_lib, os.path.join(tmp, "libishara_hip_parent_copy.so"))
    libs = dict(new=_lib.load(), parent=_foreign(os.path.abspath(args.parent_lib)), parent_again=_foreign(copy))
    nll = torch.empty(B, dtype=torch.float32, device="cuda")
    dl = torch.empty((B, T, CN), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(libs["new"].ishara_ctc_workspace_bytes(B, T, L)), dtype=torch.uint8, device="cuda")

    def call(lib):
        def run():
            if lib.ishara_ctc_loss(_lib.ptr(x), _lib.ptr(y), B, T, CN, L, CN - 1, _lib.ptr(nll), _lib.ptr(dl), C.c_float(1.0), _lib.ptr(ws), st):
                raise RuntimeError("ishara_ctc_loss failed")
        return run
    ms = _series({k: call(v) for k, v in libs.items()}, args.block, args.reps)
    shutil.rmtree(tmp)
    aa = abs(ms["parent"] - ms["parent_again"])
    return dict(shape=f"B={B} T={T} L={L} C={CN}, with dlogits", block=args.block, reps=args.reps, new_ms=ms["new"], parent_ms=ms["parent"],
                parent_again_ms=ms["parent_again"], aa_difference_ms=aa, accepted=bool(ms["new"] <= ms["parent"] + aa))


def ragged(args):
    import torch
    from ishara_amd import _lib, ctc_align, ctc_beam
    lib = _lib.load()
    x, y, fl = _inputs(B, T, CN, L)
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    lens = dict(all_T=torch.full((B,), T, dtype=torch.int32, device="cuda"), uniform_quarter_to_T=torch.from_numpy(fl).cuda())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    nll, dl, lws = f32(B), f32(B, T, CN), torch.empty(int(lib.ishara_ctc_workspace_bytes(B, T, L)), dtype=torch.uint8, device="cuda")
    idx, ln = i32(B, T), i32(B)
    W = 16
    bws = torch.empty(ctc_beam.workspace_bytes(lib, B, T, CN, W), dtype=torch.uint8, device="cuda")
    bidx, bln, bsc = i32(B, 1, T), i32(B, 1), f32(B, 1)
    aws = torch.empty(max(ctc_align.workspace_bytes(lib, B, T, L), 16), dtype=torch.uint8, device="cuda")
    fp, s0, s1, cf, sc = i32(B, T), i32(B, L), i32(B, L), f32(B, L), f32(B)
    out = {}
    for name, fl_d in lens.items():
        p = _lib.ptr
        runs = dict(
            loss=lambda: _lib.check(lib.ishara_ctc_loss_ex(p(x), p(y), B, T, CN, L, CN - 1, p(nll), p(dl), C.c_float(1.0), p(lws), p(fl_d), None, 0, st)),
            greedy=lambda: _lib.check(lib.ishara_greedy_decode_ex(p(x), B, T, CN, CN - 1, p(idx), p(ln), p(fl_d), st)),
            beam_w16=lambda: ctc_beam.launch(lib, x, B, T, CN, W, 1, None, 0.0, 0.0, bws, bidx, bln, bsc, st, frame_len=fl_d),
            align=lambda: ctc_align.launch(lib, x, y, B, T, CN, L, CN - 1, aws, fp, s0, s1, cf, sc, st, frame_len=fl_d))
        ms = {}
        for k, run in runs.items():
            ms[k + "_ms"] = _series({k: run}, 4 if k == "beam_w16" else args.block, args.reps)[k]
        out[name] = ms
    out["shape"] = f"B={B} T={T} L={L} C={CN}; beam width {W}, nbest 1"
    return out


def against_torch(args):
    import torch
    import ishara_amd
    out = {}
    for name, (b, t, c, s) in dict(small=tuple(SMALL.values()), bench=(B, T, CN, L)).items():
        x, y, fl = _inputs(b, t, c, s, seed=1)
        tl = torch.from_numpy((y != c - 1).sum(1)).cuda()
        tg = torch.from_numpy(np.where(y == c - 1, 1, y + 1)).cuda()      # blank = 0 below: classes 1 .. c - 1
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        il = torch.from_numpy(fl.astype(np.int64)).cuda()

        def ours():
            xd.grad = None
            ishara_amd.ctc_loss(xd, tg, il, tl, blank=0, reduction="mean").backward()

        def theirs():
            xd.grad = None
            torch.nn.functional.ctc_loss(torch.log_softmax(xd, -1).transpose(0, 1), tg, il, tl, blank=0, reduction="mean").backward()
        ms = _series(dict(ishara_amd=ours, torch=theirs), max(args.block // 5, 2), args.reps)
        out[name] = dict(shape=f"B={b} T={t} C={c} S={s}, lengths uniform in [T/4, T]", ishara_amd_ms=ms["ishara_amd"], torch_ms=ms["torch"],
                         note="forward + backward of reduction='mean'; torch's side includes the log_softmax its kernel needs")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libishara_hip.so built from the parent commit's csrc")
    ap.add_argument("--out", default=None)
    ap.add_argument("--block", type=int, default=50, help="launches per timed window")
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ctc_lengths_bench: no GPU (nothing is measured without one)")
    from ishara_amd.build import source_hash
    res = dict(device=torch.cuda.get_device_name(0), source_hash=source_hash(),
               timing="device events around a block of back-to-back launches, warmed up, median over the blocks; ms per launch",
               fixed_T_loss_parent_vs_new=fixed_t(a), ragged=ragged(a), against_torch=against_torch(a))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
