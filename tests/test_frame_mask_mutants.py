"""On the inputs of tests/test_frame_mask_gpu.py: each ordinary mistake of a masked mean, a masked softmax or their backward moves the fp64
restatement by at least 2x the (bf16, hence also the f32) bound the GPU test applies to some quantity of that module, so a kernel that made
it could not pass; and the per-shape bf16 bounds of frame_mask_parity.BF16_BOUND_AT are 2x a reference-side measurement."""
import numpy as np
import pytest

import frame_mask_parity as FM
import module_parity as MP
from ishara_amd import Model, make_config
from ishara_amd.model import _keras_init

# mistake -> the module kinds it can be made in
MUTANTS = {
    "mean_all_T": ("conv", "sqzconv"),             # the mean over all T frames
    "sum_over_T": ("conv", "sqzconv"),             # the masked sum divided by T
    "gate_grad_all_T": ("conv", "sqzconv"),        # the gate's gradient spread over all T frames
    "key_len_off_by_one": ("mha",),
    "next_clip_len": ("conv", "sqzconv", "mha"),   # n_{b+1} used for clip b
    "bn_valid_only": ("conv",),                    # BatchNorm statistics over the valid frames only
}
# The Squeeze-Excite gate's gradient is a small part of the ConvModule's: spread over all T frames it moves the parameter gradients by 0.8x the
# bf16 bound (rel-L2 6.9e-3) at the issue's lengths, and by 6x the f32 bound, which the GPU test applies to the same module and lengths.
# It is the f32 cases that reject this one; the bf16 bounds are not widened or narrowed for it.
F32_ONLY = {("gate_grad_all_T", "sqzconv")}
_w = {}


def weights(shape, dtype):
    """the weights test_frame_mask_gpu's model has: Model's initialisation at seed 3, perturbed (module_parity.perturbed)"""
    if (shape, dtype) not in _w:
        m = Model(make_config(**FM.SHAPES[shape], max_batch=2), device=None)
        g = np.random.default_rng(3)
        _w[shape, dtype] = MP.perturbed({n: _keras_init(n, s, g) for n, s, _, _ in m.entries}, dtype)
    return _w[shape, dtype]


_ref = {}


def _case(name, dropout, lens_id="ragged"):
    key = (name, dropout, lens_id)
    if key not in _ref:
        cfg = FM.ocfg("cfg2", dropout)
        W = weights("cfg2", "bf16")
        i, first, x, dy, seed = FM.case_inputs(cfg, name, FM.B_SMALL, "bf16", dropout)
        _ref[key] = (cfg, W, x, dy, seed, first), FM.reference(name, cfg, W, x, dy, seed, first, FM.LENS[lens_id])
    return _ref[key]


@pytest.mark.parametrize("mut,name", [(m, n) for m, kinds in sorted(MUTANTS.items()) for n in FM.MODULES if MP.module_kind(n) in kinds],
                         ids=lambda v: str(v).replace("/", "."))
def test_bounds_reject_the_mistake(mut, name):
    """the worst over the two dropout rates the GPU test runs (with drop-path a dropped clip's gate has no effect at all)"""
    kind = MP.module_kind(name)
    bound, f32 = FM.bounds(kind, "bf16", "cfg2", "ragged"), FM.bounds(kind, "f32", "cfg2")
    best, best32 = 0.0, 0.0
    for dropout in (0.0, 0.2):
        (cfg, W, x, dy, seed, first), ref = _case(name, dropout)
        bad = FM.reference(name, cfg, W, x, dy, seed, first, FM.LENS["ragged"], mut=(mut,))
        obs, _ = MP.compare(name, "bf16", FM.B_SMALL, cfg.T, bad, ref, W, bound)
        ratios = {q: obs[q] / bound[q] for q in obs if q in bound}
        print(mut, name, dropout, {q: f"{obs[q]:.3e} ({r:.1f}x)" for q, r in ratios.items()})
        best = max(best, max(ratios.values()))
        best32 = max(best32, max(obs[q] / f32[q] for q in obs if q in f32))
    assert best32 >= 2.0, f"{mut} on {name}: nothing exceeds 2x its f32 bound"
    if (mut, kind) in F32_ONLY:
        return
    assert best >= 2.0, f"{mut} on {name}: nothing exceeds 2x its bf16 bound"


@pytest.mark.parametrize("kind,shape", sorted(FM.BF16_BOUND_AT))
def test_per_shape_bounds_are_twice_the_restatement(kind, shape):
    """module_parity.BF16_BOUND_AT's rule: the entry is 2x what bf16 storage alone costs the fp64 restatement, on the GPU cases' inputs, the worst
    over the kind's modules, the entry's length sets and both dropout rates; needed (above the benchmark-shape bound); rel-L2 entries below the cap"""
    lens_ids = [shape.split("/")[1]] if "/" in shape else sorted(FM.LENS)
    worst = {}
    for name in [n for n in FM.MODULES if MP.module_kind(n) == kind]:
        for dropout in (0.0, 0.2):
            for lens_id in lens_ids:
                (cfg, W, x, dy, seed, first), ref = _case(name, dropout, lens_id)
                got = FM.reference(name, cfg, W, x, dy, seed, first, FM.LENS[lens_id], mut=("bf16_storage",))
                obs, _ = MP.compare(name, "bf16", FM.B_SMALL, cfg.T, got, ref, W, {})
                for q in FM.BF16_BOUND_AT[kind, shape]:
                    worst[q] = max(worst.get(q, 0.0), obs[q])
    print(kind, shape, {q: f"{v:.3e}" for q, v in worst.items()})
    for q, v in FM.BF16_BOUND_AT[kind, shape].items():
        assert v > MP.BF16_BOUND[kind][q], f"{q}: the per-shape entry is not needed"
        assert not q.endswith("_l2") or v <= MP.BF16_CAP
        assert abs(v - 2 * worst[q]) <= 0.03 * v, f"{q}: entry {v:.3e}, 2 x restatement {2 * worst[q]:.3e}"
