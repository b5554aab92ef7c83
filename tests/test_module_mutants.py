"""CPU: the bf16 bounds of tests/test_modules_gpu.py (module_parity.BF16_BOUND) reject ordinary mistakes.  Each mutation below is applied
to the fp64 reference of a CFG2 module (d256, T384) on the inputs the GPU test draws; the mutated result is compared with the clean one
through the GPU test's own compare(), and at least one asserted quantity must exceed its bf16 bound by 2x — so a kernel making that
mistake cannot pass.  Three tile-edge mistakes are applied at the ragged shapes of tests/test_modules_ragged_gpu.py (T = 72 / 200 / 224,
B = 2 / 8), on exactly the inputs, weights and seed its cases draw.  Also: the module list of the library's probe equals a counting walk of
the oracle's forward."""
import numpy as np
import pytest

import module_parity as MP
from ishara_amd import _lib, make_config
from ishara_amd.model import Model
from oracle import ishara_oracle as O

CFG2 = dict(dim=256, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, kernel_sizes=(11, 5, 3), num_conv_per_block=3, num_heads=8,
            expansion_factor=2, transformer_kernel_size=15, input_shape=(384, 224))
B = 2          # the smallest batch of the GPU cases


def _case(name, seed0=4242, T=384, B=B, gpu_draw=False, dropout=0.2):
    """gpu_draw: configuration, x, dy and seed as test_modules_gpu.check_module has them for this module (generator 1000 + the module's index)"""
    cfg = O.Config(dropout_rate=dropout, head_dropout=0.4 if dropout > 0 else 0.0, conformer_attn_dropout=0.1 if dropout > 0 else 0.0,
                   **{**CFG2, "input_shape": (T, 224)})
    W = MP.perturbed(O.init_params(cfg, 3), "bf16")
    g = np.random.default_rng(1000 + MP.expected_modules(cfg).index(name) if gpu_draw else 17)
    x = MP.round_to(g.standard_normal((B, cfg.T, cfg.dim)), "bf16")
    dy = None if name == "head" else MP.round_to(g.standard_normal((B, cfg.T, cfg.dim)), "bf16")
    first = FIRST_SITE[name]
    seed = MP.mixed_droppath_seed(seed0, first, B, dropout) if MP.module_kind(name) == "conv" and dropout > 0 else seed0
    return cfg, W, x, dy, seed, first


FIRST_SITE = {n: s for n, s, _ in MP.walk_sites(O.Config(dropout_rate=0.2, **CFG2))}

# mutation -> (module, the quantities that must see it; None: any)
MUTANTS = {
    "eca_gate_const": ("convsqueeze_0_1", None),
    "bn_stats_const": ("convsqueeze_0_1", None),
    "bias_grad_no_droppath": ("convsqueeze_0_1", None),
    "gate_other_sample": ("convsqueeze_0_1", ("y_l2", "dx_l2")),          # one sample wrong: the per-sample metric
    "eca_wrap": ("convsqueeze_0_1", ("y_elem", "dx_elem", "grad_max")),   # a few edge channels wrong: the elementwise (max-abs) bounds
    "ln_bwd_no_residual": ("squeezeformer_0/ffn1", None),
    "ffn_mask_not_in_bwd": ("squeezeformer_0/ffn1", None),
}


@pytest.mark.parametrize("name,T", [pytest.param(n, T, id=n + ("" if T == 384 else f"-t{T}")) for T in (384, 200)
                                    for n in ("convsqueeze_0_1", "squeezeformer_0/ffn1", "conformer_0/ffn2")])
def test_unmutated_restatement_is_the_oracle(name, T):
    """the switchable restatements in module_parity compute what the oracle's module functions do when nothing is switched on (fp64 rounding apart)"""
    cfg, W, x, dy, seed, first = _case(name, T=T)
    a = MP.reference(name, cfg, W, x, dy, seed, first)
    b = MP.reference(name, cfg, W, x, dy, seed, first, mut=("none",))
    assert np.allclose(a["y"], b["y"], rtol=1e-12, atol=1e-12) and np.allclose(a["dx"], b["dx"], rtol=1e-11, atol=1e-11)
    for k in a["grads"]:
        assert np.allclose(a["grads"][k], b["grads"][k], rtol=1e-10, atol=1e-12), k


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_bf16_bounds_reject_the_mutant(mut):
    name, must = MUTANTS[mut]
    cfg, W, x, dy, seed, first = _case(name)
    ref = MP.reference(name, cfg, W, x, dy, seed, first)
    bad = MP.reference(name, cfg, W, x, dy, seed, first, mut=(mut,))
    bound = MP.bounds(MP.module_kind(name), "bf16")
    obs, _ = MP.compare(name, "bf16", B, cfg.T, bad, ref, W, bound)
    ratios = {q: obs[q] / bound[q] for q in obs if q in bound and (must is None or q in must)}
    print(mut, {q: f"{obs[q]:.3e} ({r:.1f}x)" for q, r in ratios.items()})
    assert max(ratios.values()) >= 2.0, f"{mut}: no asserted quantity exceeds 2x its bf16 bound: observed {obs}, bounds {bound}"


# the shapes of tests/test_modules_ragged_gpu.py: id -> (T, B)
RAGGED = {"t72": (72, 2), "t200": (200, 2), "t224": (224, 2), "t200b8": (200, 8)}
# tile-edge mutation -> (modules, shapes at which it is not vacuous, the quantities that must see it)
RAGGED_MUTANTS = {
    "droppath_by_fragment": (["convsqueeze_0_1"], ["t72", "t200", "t200b8"], ("y_elem", "y_l2")),       # T % 16 == 0 at t224: every fragment inside one sample
    "wgrad_tail_rows_dropped": (["convsqueeze_0_1", "squeezeformer_0/ffn1"], ["t72", "t200", "t224", "t200b8"], ("grad_l2", "grad_max")),
    "bn_stats_skip_tail": (["convsqueeze_0_1"], ["t72", "t200", "t224", "t200b8"], ("stat",)),
}
_ragged_ref = {}


def _ragged_case(name, shape):
    """the GPU case's inputs and its clean fp64 reference, computed once per (module, shape)"""
    if (name, shape) not in _ragged_ref:
        T, Bn = RAGGED[shape]
        case = _case(name, T=T, B=Bn, gpu_draw=True)
        _ragged_ref[name, shape] = case, MP.reference(name, *case)
    return _ragged_ref[name, shape]


@pytest.mark.parametrize("mut,name,shape", [(m, n, s) for m, (names, shapes, _) in sorted(RAGGED_MUTANTS.items()) for n in names for s in shapes],
                         ids=lambda v: str(v).replace("/", "."))
def test_bf16_bounds_reject_the_tile_edge_mutant(mut, name, shape):
    """a kernel that took the drop-path scale per 16-row fragment, left the last partial 64-row tile out of a weight gradient, or took the
    BatchNorm statistics over whole 32-step segments only cannot pass tests/test_modules_ragged_gpu.py: on that test's inputs the named
    quantities exceed 2x their bf16 bound"""
    must = RAGGED_MUTANTS[mut][2]
    (cfg, W, x, dy, seed, first), ref = _ragged_case(name, shape)
    Bn = RAGGED[shape][1]
    if mut == "droppath_by_fragment":       # not vacuous: two neighbouring samples with different draws share a fragment
        keep = MP.rng.keep_mask(seed, first, Bn, 1, 0.2)[:, 0]
        assert any(keep[b] != keep[b - 1] and (b * cfg.T) % 16 for b in range(1, Bn)), keep
    bad = MP.reference(name, cfg, W, x, dy, seed, first, mut=(mut,))
    bound = MP.bounds(MP.module_kind(name), "bf16", shape)
    obs, _ = MP.compare(name, "bf16", Bn, cfg.T, bad, ref, W, bound)
    ratios = {q: obs[q] / bound[q] for q in must}
    print(mut, name, shape, {q: f"{obs[q]:.3e} ({r:.1f}x)" for q, r in ratios.items()})
    assert max(ratios.values()) >= 2.0, f"{mut}: none of {must} exceeds 2x its bf16 bound: observed {obs}, bounds {bound}"


# the dropout rates tests/test_modules_ragged_gpu.py runs in bf16 at each shape
RAGGED_DROPOUTS = {"t72": (0.2,), "t200": (0.2, 0.0), "t224": (0.2, 0.0), "t200b8": (0.2,)}


@pytest.mark.parametrize("kind,shape", sorted(MP.BF16_BOUND_AT))
def test_per_shape_bounds_are_twice_the_restatement(kind, shape):
    """every per-shape bf16 bound is 2x what bf16 storage alone costs on the reference side: the module restated in fp64 with its stored
    activations rounded to bf16 against the clean fp64 reference, on the GPU cases' inputs, the worst over the kind's modules and dropout rates"""
    T, Bn = RAGGED[shape]
    worst = {}
    for name in [n for n in MP.expected_modules(O.Config(**CFG2)) if MP.module_kind(n) == kind]:
        for dropout in RAGGED_DROPOUTS[shape]:
            cfg, W, x, dy, seed, first = _case(name, T=T, B=Bn, gpu_draw=True, dropout=dropout)
            labels = O.synthetic_batch(cfg, Bn, seed=2)[1] if kind == "head" else None
            ref = MP.reference(name, cfg, W, x, dy, seed, first, labels=labels)
            got = MP.reference(name, cfg, W, x, dy, seed, first, labels=labels, mut=("bf16_storage",))
            obs, _ = MP.compare(name, "bf16", Bn, T, got, ref, W, {})
            for q in MP.BF16_BOUND_AT[kind, shape]:
                worst[q] = max(worst.get(q, 0.0), obs[q])
    print(kind, shape, {q: f"{v:.3e}" for q, v in worst.items()})
    for q, v in MP.BF16_BOUND_AT[kind, shape].items():
        assert v > MP.BF16_BOUND[kind][q], f"{q}: the per-shape entry is not needed"
        assert abs(v - 2 * worst[q]) <= 0.03 * v, f"{q}: entry {v:.3e}, 2 x restatement {2 * worst[q]:.3e}"


@pytest.mark.parametrize("kw", [
    dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1),
    dict(dim=256, input_shape=(384, 224)),
    dict(dim=256, num_conv_squeeze_blocks=4, num_conv_conform_blocks=4, num_conv_per_block=0, squeeze_expansion=4, conformer_expansion=2, top_dim=256),
])
def test_module_info_matches_a_walk_of_the_oracle(kw):
    """names, order, first dropout site and site count of ishara_debug_module_info on a device-less handle against the oracle's own site
    counter; in / out widths against the configuration"""
    m = Model(make_config(**kw, max_batch=2), device=None)
    cfg = O.Config(**kw)
    walk = MP.walk_sites(cfg)
    assert [n for n, _, _ in walk] == MP.expected_modules(cfg)
    assert m.module_names() == [n for n, _, _ in walk]
    assert int(m._lib.ishara_debug_module_count(m._h)) == len(walk)
    for i, (n, s0, ns) in enumerate(walk):
        name, cin, cout, first, count = m._module_info(i)
        assert (name, first, count) == (n, s0, ns), (i, name, first, count, n, s0, ns)
        assert cin == (cfg.F if n == "stem" else cfg.dim) and cout == (cfg.num_classes if n == "head" else cfg.dim)
    with pytest.raises(_lib.IsharaError):
        m._module_info(len(walk))
