"""CPU: which depthwise-conv kernel a call runs on, read from the route itself (ishara_debug_dwconv_kernel_name: host only, nothing is
launched).  The expectations were derived from the launchers as they were before dwconv_fwd_route / dwconv_bwd_route existed
(three inline if-chains), not from the route functions."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = 0, 1, 2
STATS, SCR, BN = 1, 2, 4                      # flag bits
FORCE_LDS = 4                                 # ishara_debug_force_regstage: the LDS-tiled depthwise kernels

STREAM, REG8, REG = "dwconv_stream_kernel", "dwconv_reg8_kernel", "dwconv_reg_kernel"
TILE11, TILE15, TILE31 = "dwconv_kernel<11,11>", "dwconv_kernel<0,15>", "dwconv_kernel<0,31>"
FUSED_BN, FUSED = "dwconv_bwd_fused_kernel<BN>", "dwconv_bwd_fused_kernel"
WIN, TILE_PART, TILE_ATOMIC = "dwconv_wgrad_win_kernel", "dwconv_wgrad_kernel<part>", "dwconv_wgrad_kernel<atomic>"


def tile_of(k):
    return TILE11 if k == 11 else (TILE15 if k <= 15 else TILE31)


# (dt, B, T, C, k, statistics, scratch) -> kernel
FWD = [
    ((BF16, 256, 384, 512, 11, 1, 1), STREAM),
    ((F16, 9, 64, 128, 15, 0, 0), STREAM),
    ((BF16, 8, 384, 512, 11, 1, 1), TILE11),          # B <= 8
    ((BF16, 9, 40, 128, 11, 1, 1), TILE11),           # T < 64
    ((BF16, 9, 384, 512, 11, 1, 0), TILE11),          # statistics only through partial rows
    ((BF16, 256, 384, 512, 5, 1, 1), REG8),
    ((BF16, 256, 384, 512, 3, 1, 1), REG8),
    ((BF16, 1, 384, 512, 5, 0, 0), REG8),
    ((BF16, 2, 64, 512, 5, 1, 0), REG),
    ((F32, 2, 64, 512, 5, 1, 1), REG),
    ((BF16, 2, 64, 128, 3, 1, 1), REG),               # C / 8 < 32
    ((BF16, 2, 64, 384, 5, 1, 1), TILE15),
    ((F32, 9, 384, 512, 11, 1, 1), TILE11),
    ((BF16, 2, 104, 32, 15, 1, 1), TILE15),
    ((BF16, 1, 16, 512, 31, 0, 0), TILE31),
]
# (dt, C, k, scratch, BatchNorm) -> kernel(s)
BWD = [
    ((BF16, 512, 11, 1, 1), FUSED_BN),
    ((BF16, 512, 5, 1, 1), FUSED_BN),
    ((BF16, 512, 15, 1, 1), FUSED),                   # BatchNorm not folded: launch_dwconv_bwd_bn answers 0
    ((BF16, 512, 15, 1, 0), FUSED),
    ((BF16, 512, 11, 1, 0), FUSED),
    ((BF16, 512, 5, 1, 0), FUSED),
    ((BF16, 512, 3, 1, 0), FUSED),
    ((BF16, 384, 5, 1, 0), FUSED),
    ((F32, 512, 5, 1, 0), FUSED),
    ((F32, 512, 11, 1, 0), TILE11 + "+" + WIN),
    ((F32, 512, 11, 1, 1), TILE11 + "+" + WIN),       # BatchNorm not folded
    ((BF16, 2048, 5, 1, 0), TILE15 + "+" + WIN),
    ((BF16, 64, 7, 1, 0), TILE15 + "+" + TILE_PART),
    ((BF16, 64, 7, 0, 0), TILE15 + "+" + TILE_ATOMIC),
    ((BF16, 512, 5, 0, 0), REG + "+" + TILE_ATOMIC),
]


def fwd_name(lib, dt, B, T, C, k, stats, scr):
    return lib.ishara_debug_dwconv_kernel_name(dt, 0, B, T, C, k, k - 1, (STATS if stats else 0) | (SCR if scr else 0)).decode()


def bwd_name(lib, dt, C, k, scr, bn):
    return lib.ishara_debug_dwconv_kernel_name(dt, 1, 4, 96, C, k, k - 1, (SCR if scr else 0) | (BN if bn else 0)).decode()


@pytest.fixture
def force_lds(lib):
    lib.ishara_debug_force_regstage(FORCE_LDS)
    yield
    lib.ishara_debug_force_regstage(0)


@pytest.mark.parametrize("case,want", FWD)
def test_forward_route(lib, case, want):
    assert fwd_name(lib, *case) == want


@pytest.mark.parametrize("case,want", BWD)
def test_backward_route(lib, case, want):
    assert bwd_name(lib, *case) == want


@pytest.mark.parametrize("B,T,C,k", [(2, 64, 512, 32), (2, 64, 512, 0), (2, 64, 12, 5)])
def test_refused_shapes_have_no_kernel(lib, B, T, C, k):
    for backward in (0, 1):
        assert lib.ishara_debug_dwconv_kernel_name(BF16, backward, B, T, C, k, max(k - 1, 0), STATS | SCR) == b""


def test_forced_lds_takes_the_tile_kernels(lib, force_lds):
    for case, _ in FWD:
        assert fwd_name(lib, *case) == tile_of(case[4]), case
    for (dt, C, k, _, bn), _ in BWD:
        for scr in (0, 1):
            assert bwd_name(lib, dt, C, k, scr, bn) == tile_of(k) + "+" + TILE_ATOMIC, (dt, C, k, scr, bn)


def test_no_dw_stream_switch_takes_the_tile_kernel():
    """ISHARA_NO_DW_STREAM is read once per process: a fresh child."""
    code = "from ishara_amd import _lib; print(_lib.load().ishara_debug_dwconv_kernel_name(1, 0, 256, 384, 512, 11, 10, 3).decode())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**os.environ, "ISHARA_NO_DW_STREAM": "1"}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == TILE11
