"""CPU: the launch plan of a Conv1DBlock, read from the plan itself (ishara_debug_conv_block_route_name: host only, nothing is launched).
The expectations were derived by hand from conv_fwd / conv_bwd as they were before conv_block_plan existed (three if-ladders over
infer_fused / train_fused / fl / prows, the inline `folded` and `psa` conditions, and the backward's second decision from ds.thr,
cb.folded, cb.psa, r.key_len and the answer of launch_dwconv_bwd_bn), not from the new function.

Name: "forward|backward".  forward = the BatchNorm constants' source (part: the depthwise conv's partial rows; sums: per-sample sums after
stats_reduce; infer: none, the inference gate forms them), "+len" (masked_time_mean + eca_fwd_len), "+fold" (drop-path scale folded into
P, Q), "+prologue" | "+affine" (sample_affine + GEMM), "+psa" (h4 not written).  backward = psa | folded | scaled_copy | plain, then
len | fused_bn | two_kernel; "-" at inference.  Everything but psa runs sample_reduce."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = 0, 1, 2
DROP, LEN, PSA = 1, 2, 4                      # flag bits
B_NO_PSA = 11                                 # tests/test_modules_gpu.py: no split of whole samples with at most 8 per split

# (dt, training, B, T, d, k, flags) -> route.  d 256, T 384: configs[1] of the benchmark (project conv K = 512 -> N = 256)
ROUTES = [
    ((BF16, 1, 64, 384, 256, 11, DROP | PSA), "part+fold+prologue+psa|psa+fused_bn"),
    ((BF16, 1, 64, 384, 256, 11, PSA), "part+prologue+psa|psa+fused_bn"),
    ((BF16, 1, 64, 384, 256, 5, DROP | PSA), "part+fold+prologue+psa|psa+fused_bn"),
    # frame lengths: BatchNorm still from the partial rows, the length gate, no psa, bn_bwd_apply_len + plain depthwise backward
    ((BF16, 1, 64, 384, 256, 11, DROP | LEN | PSA), "part+len+fold+prologue|folded+len"),
    ((BF16, 1, 64, 384, 256, 11, LEN | PSA), "part+len+prologue|plain+len"),
    # psa switched off (ISHARA_NO_PSA, or an f32 model): h4 written by the prologue, sample_reduce
    ((BF16, 1, 64, 384, 256, 11, DROP), "part+fold+prologue|folded+fused_bn"),
    ((BF16, 1, 64, 384, 256, 11, 0), "part+prologue|plain+fused_bn"),
    # f32: no fold (bf16 only), no prologue (16-bit only), k 11 has no fp32 one-pass depthwise backward
    ((F32, 1, 64, 384, 256, 11, DROP), "part+affine|scaled_copy+two_kernel"),
    ((F32, 1, 64, 384, 256, 11, 0), "part+affine|plain+two_kernel"),
    ((F32, 1, 64, 384, 256, 5, DROP), "part+affine|scaled_copy+fused_bn"),
    # k 15: the one-pass depthwise backward does not carry the BatchNorm
    ((BF16, 1, 64, 384, 256, 15, DROP | PSA), "part+fold+prologue+psa|psa+two_kernel"),
    # gemm_tn_psa_ok refuses the batch; fold and prologue do not depend on it
    ((BF16, 1, B_NO_PSA, 384, 256, 11, DROP | PSA), "part+fold+prologue|folded+fused_bn"),
    ((BF16, 1, B_NO_PSA, 384, 256, 11, PSA), "part+prologue|plain+fused_bn"),
    # inference: the fused gate; with lengths bn_finalize from the summed statistics and the length gate
    ((BF16, 0, 1, 384, 256, 11, PSA), "infer+prologue|-"),
    ((F16, 0, 1, 384, 256, 11, 0), "infer+prologue|-"),
    ((F16, 0, 1, 384, 256, 5, 0), "infer+prologue|-"),
    ((F32, 0, 1, 384, 256, 11, 0), "infer+affine|-"),
    ((BF16, 0, 1, 384, 256, 11, LEN | PSA), "sums+len+prologue|-"),
    # project conv K = 384: no prologue (K 256 / 512 / 1024), no fold, no psa
    ((BF16, 1, 4, 384, 192, 5, DROP | PSA), "part+affine|scaled_copy+fused_bn"),
    ((BF16, 1, 4, 384, 192, 5, PSA), "part+affine|plain+fused_bn"),
    # T % 64 != 0 (tests/test_modules_ragged_gpu.py t200): a workgroup's rows would straddle samples, T % 32 != 0 rules out the fold
    ((BF16, 1, 2, 200, 256, 11, DROP | PSA), "part+affine|scaled_copy+fused_bn"),
]


def name(lib, dt, training, B, T, d, k, flags):
    return lib.ishara_debug_conv_block_route_name(dt, training, B, T, d, k, flags).decode()


@pytest.mark.parametrize("case,want", ROUTES)
def test_route(lib, case, want):
    assert name(lib, *case) == want


def test_the_affine_row_is_refused_by_the_prologue_test(lib):
    """K = 384: the A-stationary kernel does not take the project GEMM at all (the plain Dense of that shape runs on another kernel), and
    gemm_nt_as_prologue_ok asks gemm_nt_as_applicable before anything else; at K = 512 the same call is an A-stationary one"""
    assert not lib.ishara_debug_dense_kernel_name(BF16, 4 * 384, 384, 192, 0, 1).decode().startswith("gemm_nt_as")
    assert lib.ishara_debug_dense_kernel_name(BF16, 4 * 384, 512, 256, 0, 1).decode().startswith("gemm_nt_as")


@pytest.mark.parametrize("case", [(BF16, 1, 2, 64, 256, 32, 0), (BF16, 1, 2, 64, 256, 0, 0), (BF16, 1, 2, 64, 6, 5, 0), (F16, 1, 2, 64, 256, 5, 0),
                                  (F16, 0, 2, 64, 256, 5, LEN), (BF16, 0, 2, 64, 256, 5, DROP), (7, 0, 2, 64, 256, 5, 0), (BF16, 1, 0, 64, 256, 5, 0)])
def test_refused_calls_have_no_route(lib, case):
    assert name(lib, *case) == ""


def test_forced_tile_gemm_takes_neither_fold_nor_prologue(lib):
    lib.ishara_debug_force_regstage(8192)
    try:
        assert name(lib, BF16, 1, 64, 384, 256, 11, DROP | PSA) == "part+affine|scaled_copy+fused_bn"
        assert name(lib, BF16, 0, 1, 384, 256, 11, PSA) == "infer+affine|-"
    finally:
        lib.ishara_debug_force_regstage(0)


def _child(env, args):
    code = f"from ishara_amd import _lib; print(_lib.load().ishara_debug_conv_block_route_name{args}.decode())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**os.environ, env: "1"}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


def test_no_infer_fusion_switch_takes_the_summed_statistics():
    """a fresh child, as for ISHARA_NO_DW_STREAM (tests/test_dwconv_route.py): stats_reduce + bn_finalize + the plain gate"""
    assert _child("ISHARA_NO_INFER_FUSION", (BF16, 0, 1, 384, 256, 11, PSA)) == "sums+prologue|-"


def test_no_stats_fusion_switch_takes_the_summed_statistics():
    """ISHARA_NO_STATS_FUSION is read once per process: a fresh child.  Only the statistics change"""
    assert _child("ISHARA_NO_STATS_FUSION", (BF16, 1, 64, 384, 256, 11, DROP | PSA)) == "sums+fold+prologue+psa|psa+fused_bn"
    assert _child("ISHARA_NO_STATS_FUSION", (BF16, 1, 64, 384, 256, 11, LEN | PSA)) == "sums+len+prologue|plain+len"
