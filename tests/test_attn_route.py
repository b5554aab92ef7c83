"""CPU: which attention kernel a call runs on, read from the route itself (ishara_debug_attn_kernel_name: host only, nothing is launched).
The expectations were derived from the launchers as they were before attn_fwd_route / attn_bwd_route existed (launch_attn_fwd / _bwd and the
three launch_attn_*_mfma* launchers, each with its own tests), not from the route functions.  The one row that differs from them on purpose:
an fp16 backward is refused (it used to run the fp32 kernels on fp16 data)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = 0, 1, 2
DROP, BITS, HEAD_MAJOR = 1, 2, 4              # flag bits
TWO_PASS = 1 << 16                            # ishara_debug_force_regstage: the two-kernel attention backward

FWD_MFMA, FWD_LANE = "attn_fwd_mfma_kernel", "attn_fwd_kernel"
FUSED = "attn_bwd_fused_kernel"
PAIR_MFMA = "attn_bwd_dq_mfma_kernel + attn_bwd_dkv_mfma_kernel"
PAIR_LANE = "attn_bwd_dq_kernel + attn_bwd_dkv_kernel"

# (dt, T, dh, impl, dropout, keep-bit buffer) -> kernel
FWD = [
    ((BF16, 384, 32, 1, 1, 1), FWD_MFMA + "<32,2>"),
    ((BF16, 384, 32, 1, 1, 0), FWD_MFMA + "<32,1>"),
    ((BF16, 384, 32, 1, 0, 1), FWD_MFMA + "<32,0>"),
    ((BF16, 136, 64, 1, 1, 1), FWD_MFMA + "<64,2>"),
    ((BF16, 100, 32, 1, 1, 1), ""),                          # bf16 at T % 8 != 0 is refused ...
    ((F16, 384, 32, 1, 0, 0), FWD_MFMA + "<32,0,f16>"),
    ((F16, 100, 32, 1, 0, 0), FWD_LANE + "<f16,8>"),         # ... where fp16 falls back to the lane-split kernel
    ((F16, 384, 32, 1, 1, 0), FWD_LANE + "<f16,8>"),         # the fp16 MFMA kernel has no dropout
    ((F32, 64, 16, 1, 0, 0), FWD_LANE + "<float,4>"),
    ((BF16, 64, 16, 1, 1, 1), FWD_LANE + "<bf16,4>"),
    ((BF16, 384, 32, 0, 1, 1), FWD_LANE + "<bf16,8>"),
    ((BF16, 64, 40, 1, 0, 0), ""),
    ((F32, 64, 40, 0, 0, 0), ""),
]
# (dt, T, dh, impl, dropout, keep-bit buffer, head-major dqkv) -> kernel(s)
BWD = [
    ((BF16, 128, 32, 1, 1, 1, 1), FUSED + "<8,1,2,FULL>"),
    ((BF16, 136, 32, 1, 1, 1, 1), FUSED + "<12,1,2,ragged>"),
    ((BF16, 192, 32, 1, 1, 1, 1), FUSED + "<12,1,2,FULL>"),
    ((BF16, 200, 32, 1, 1, 1, 1), FUSED + "<8,2,2,ragged>"),
    ((BF16, 256, 32, 1, 1, 1, 1), FUSED + "<8,2,2,FULL>"),
    ((BF16, 264, 32, 1, 1, 1, 1), FUSED + "<12,2,2,ragged>"),
    ((BF16, 384, 32, 1, 1, 1, 1), FUSED + "<12,2,2,FULL>"),
    ((BF16, 392, 32, 1, 1, 1, 1), PAIR_MFMA + "<32,2>"),
    ((BF16, 136, 64, 1, 1, 1, 1), PAIR_MFMA + "<64,2>"),
    ((BF16, 384, 32, 1, 1, 0, 1), FUSED + "<12,2,1,FULL>"),
    ((BF16, 392, 32, 1, 1, 0, 1), PAIR_MFMA + "<32,1>"),
    ((BF16, 384, 32, 1, 0, 1, 1), FUSED + "<12,2,0,FULL>"),
    ((BF16, 136, 64, 1, 0, 1, 1), PAIR_MFMA + "<64,0>"),
    ((BF16, 384, 32, 1, 1, 1, 0), PAIR_LANE + "<bf16,8>"),   # not head-major
    ((BF16, 384, 32, 0, 1, 1, 1), PAIR_LANE + "<bf16,8>"),
    ((BF16, 65, 24, 1, 1, 1, 1), PAIR_LANE + "<bf16,6>"),
    ((F32, 384, 32, 1, 1, 1, 1), PAIR_LANE + "<float,8>"),
    ((F32, 33, 64, 0, 0, 0, 1), PAIR_LANE + "<float,16>"),
    ((BF16, 100, 32, 1, 1, 1, 1), ""),
    ((BF16, 64, 40, 1, 1, 1, 1), ""),
    ((F16, 384, 32, 1, 0, 0, 1), ""),
    ((F16, 64, 16, 0, 0, 0, 1), ""),
]


def fwd_name(lib, dt, T, dh, impl, drop, bits):
    return lib.ishara_debug_attn_kernel_name(dt, 0, T, dh, impl, (DROP if drop else 0) | (BITS if bits else 0)).decode()


def bwd_name(lib, dt, T, dh, impl, drop, bits, hm):
    return lib.ishara_debug_attn_kernel_name(dt, 1, T, dh, impl, (DROP if drop else 0) | (BITS if bits else 0) | (HEAD_MAJOR if hm else 0)).decode()


@pytest.fixture
def two_pass(lib):
    lib.ishara_debug_force_regstage(TWO_PASS)
    yield
    lib.ishara_debug_force_regstage(0)


@pytest.mark.parametrize("case,want", FWD)
def test_forward_route(lib, case, want):
    assert fwd_name(lib, *case) == want


@pytest.mark.parametrize("case,want", BWD)
def test_backward_route(lib, case, want):
    assert bwd_name(lib, *case) == want


def test_forced_two_pass_takes_the_kernel_pair(lib, two_pass):
    fused = 0
    for case, want in BWD:
        if want.startswith(FUSED):
            dm = want.split(",")[2]
            want, fused = f"{PAIR_MFMA}<{case[2]},{dm}>", fused + 1
        assert bwd_name(lib, *case) == want, case
    assert fused == 9
    for case, want in FWD:                     # the switch is the backward's alone
        assert fwd_name(lib, *case) == want, case


def test_no_attn_bits_switch_hashes_in_both_passes():
    """ISHARA_NO_ATTN_BITS is read once per process: a fresh child.  Every row that is given the keep-bit buffer answers dropout mode 1."""
    rows = [(0, c) for c, w in FWD if c[4] and c[5] and "mfma" in w] + [(1, c) for c, w in BWD if c[4] and c[5] and (FUSED in w or PAIR_MFMA in w)]
    assert len(rows) == 11
    code = ("import sys; from ishara_amd import _lib; L = _lib.load()\n"
            "for a in sys.argv[1:]:\n"
            "    b, dt, T, dh, impl, fl = map(int, a.split(','))\n"
            "    print(L.ishara_debug_attn_kernel_name(dt, b, T, dh, impl, fl).decode())\n")
    args = [f"{b},{c[0]},{c[1]},{c[2]},{c[3]},{DROP | BITS | HEAD_MAJOR}" for b, c in rows]
    r = subprocess.run([sys.executable, "-c", code, *args], cwd=ROOT, env={**os.environ, "ISHARA_NO_ATTN_BITS": "1"}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]
    want = {0: dict(FWD), 1: dict(BWD)}
    assert len(got) == len(rows)
    for (b, c), name in zip(rows, got):
        clean = want[b][c]
        head, _, tail = clean.rpartition(",2")      # <32,2> -> <32,1>; <12,2,2,FULL> -> <12,2,1,FULL>
        assert name == head + ",1" + tail and name != clean, (b, c, name)
