"""CPU: the bf16 bounds of tests/test_modules_gpu.py (module_parity.BF16_BOUND) reject ordinary mistakes.  Each mutation below is applied
to the fp64 reference of a CFG2 module (d256, T384) on the inputs the GPU test draws; the mutated result is compared with the clean one
through the GPU test's own compare(), and at least one asserted quantity must exceed its bf16 bound by 2x — so a kernel making that
mistake cannot pass.  Also: the module list of the library's probe equals a counting walk of the oracle's forward."""
import numpy as np
import pytest

import module_parity as MP
from ishara_amd import _lib, make_config
from ishara_amd.model import Model
from oracle import ishara_oracle as O

CFG2 = dict(dim=256, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, kernel_sizes=(11, 5, 3), num_conv_per_block=3, num_heads=8,
            expansion_factor=2, transformer_kernel_size=15, input_shape=(384, 224))
B = 2          # the smallest batch of the GPU cases


def _case(name, seed0=4242):
    cfg = O.Config(dropout_rate=0.2, **CFG2)
    W = MP.perturbed(O.init_params(cfg, 3), "bf16")
    g = np.random.default_rng(17)
    x = MP.round_to(g.standard_normal((B, cfg.T, cfg.dim)), "bf16")
    dy = MP.round_to(g.standard_normal((B, cfg.T, cfg.dim)), "bf16")
    first = FIRST_SITE[name]
    seed = MP.mixed_droppath_seed(seed0, first, B, 0.2) if MP.module_kind(name) == "conv" else seed0
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


@pytest.mark.parametrize("name", ["convsqueeze_0_1", "squeezeformer_0/ffn1", "conformer_0/ffn2"])
def test_unmutated_restatement_is_the_oracle(name):
    """the switchable restatements in module_parity compute what the oracle's module functions do when nothing is switched on (fp64 rounding apart)"""
    cfg, W, x, dy, seed, first = _case(name)
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
