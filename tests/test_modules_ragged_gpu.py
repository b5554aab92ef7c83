"""Every module of the Keras hybrid alone against fp64 at sequence lengths that are no multiple of 128.

tests/test_modules_gpu.py runs T = 384 / 512 only, where every row count M = B * T is a multiple of 128 and every predicate the fast path
picks its kernels by is true.  The shapes below are the smallest that make each of them false (the body and the metrics are
test_modules_gpu.check_module and module_parity's; the bounds: see below):

  t72        T  72, B 2, M  144   M < 256: the register weight-gradient GEMM everywhere; the widest column split of the A-stationary GEMM;
                                  64-row workgroups with a 16-row tail; the MFMA fragment at row 64 straddles two samples; attention at T % 16 == 8
  t200       T 200, B 2, M  400   M % 64 == 16, T % 32 == 8: no drop-path fold (gemm_tn_bias_rowscale_ok), no per-sample-affine prologue
                                  (gemm_nt_as_prologue_ok: T % BR), no transposed-read weight gradient (tn_tr_takes); 16-row tail; the fragment at
                                  row 192 straddles two samples; depthwise backward segments 6.25 x 32 and 4.17 x 48
  t224       T 224, B 2, M  448   M % 64 == 0, T % 32 == 0, T % 64 == 32: drop-path folded without the affine prologue; the weighted-bias-sum
                                  transposed-read weight gradient at T % 128 != 0
  t200b8     T 200, B 8, M 1600   M > AS_SMALL_M: 128-row workgroups at K = 256 with a 64-row tail, no column split; the transposed-read
                                  weight gradient with a short last M-split and no fold
  d512_t200  T 200, B 2, M  400   the d512 model: the K = 1024 project conv (128-row workgroups, 16-row tail), the K = 512 LayerNorm path

The routes asserted from the profile report (bf16) follow from those predicates: see _check_routes.

Bounds: module_parity.bounds(kind, dtype) as at the benchmark's shapes, but for three quantities that average bf16 storage rounding over
the B * T rows and have far fewer rows here — a Conv1DBlock's implied batch statistics at t72, the head's CTC loss at t72 / t200 / t224 and
the top_conv/kernel gradient at t224 with dropout.  They are held to 2x what an fp64 restatement of the module with bf16-rounded stored
activations loses against clean fp64 (module_parity.BF16_BOUND_AT, derived and re-checked on the CPU by tests/test_module_mutants.py; the
MI355X matches that restatement to three digits, and the f32 cases of the same shapes hold 2e-4)."""
import pytest

import module_parity as MP
import test_modules_gpu as TM

pytestmark = pytest.mark.gpu

# id -> (base of TM.SHAPES, T, B)
RAGGED = {"t72": ("cfg2", 72, 2), "t200": ("cfg2", 200, 2), "t224": ("cfg2", 224, 2), "t200b8": ("cfg2", 200, 8), "d512_t200": ("d512", 200, 2)}
NO_TR = ("t72", "t200", "d512_t200")      # tn_tr_takes is false: M < 256 or M % 64 != 0
TR = ("t224", "t200b8")
D512_MODULES = ["convsqueeze_0_1", "squeezeformer_0/ffn1", "squeezeformer_0/mha", "conformer_0/conv", "head"]


def _kw(shape):
    base, T, _ = RAGGED[shape]
    return dict(TM.SHAPES[base], input_shape=(T, TM.SHAPES[base]["input_shape"][1]))


def _cases():
    out = []

    def add(shape, dtype, dropout, names):
        out.extend((shape, dtype, dropout, n) for n in names)

    for shape in ("t72", "t200", "t224", "t200b8"):
        add(shape, "bf16", 0.2, TM.ALL)
    for shape in ("t200", "t224"):
        add(shape, "bf16", 0.0, TM.NO_ATTN)
    for shape in ("t72", "t200"):
        add(shape, "f32", 0.2, TM.ALL)
    add("t224", "f32", 0.2, ["head"])      # the f32 counterpart of the bf16 case whose top_conv/kernel gradient and loss carry a per-shape bound
    add("d512_t200", "bf16", 0.2, D512_MODULES)
    return out


def _check_routes(name, kind, shape, dtype, dropout, B, variant, report):
    """The kernels each ragged shape is meant to reach, by their names in the profile report (bf16 only)."""
    if dtype != "bf16":
        return
    pro = MP.prologue_kinds(report)
    if kind in ("ffn", "sqzconv") or (kind == "mha" and RAGGED[shape][0] == "cfg2"):
        assert 1 in pro, f"no A-stationary GEMM with the LayerNorm prologue in {report}"
    if kind == "conv":
        assert "dwconv_bwd" in report and "bn_bwd_apply" not in report, f"not the fused depthwise / BatchNorm backward: {report}"
        # gemm_nt_as_prologue_ok: the per-sample-affine prologue needs T % BR == 0 (BR = 64 / 128 rows per workgroup); none of these T has it
        assert 2 not in pro, f"a per-sample-affine prologue at T % BR != 0: {report}"
        assert "sample_affine" in report, f"no separate per-sample affine pass: {report}"
        assert TM.PSA_KEY not in report, f"the per-sample-affine weight gradient at T % 128 != 0: {report}"
        assert "sample_reduce" in report, report
    tr = [k for k in report if k.startswith("gemm_tn_tr_kernel") or k.startswith("gemm_tn_big_kernel")]
    if shape in NO_TR:
        assert not tr, f"a transposed-read weight-gradient GEMM at M = {B * RAGGED[shape][1]} (tn_tr_takes): {report}"
    if shape in TR and kind in ("conv", "ffn"):
        assert "gemm_tn_tr_kernel<0>" in report, f"no transposed-read weight-gradient GEMM: {report}"


@pytest.mark.parametrize("shape,dtype,dropout,name", _cases(), ids=lambda v: str(v).replace("/", ".") if not isinstance(v, float) else f"drop{v}")
def test_module_matches_fp64_at_ragged_T(shape, dtype, dropout, name):
    TM.check_module(shape, dtype, dropout, RAGGED[shape][2], "", name, kw=_kw(shape), log_test="module_ragged", check_routes=_check_routes)
