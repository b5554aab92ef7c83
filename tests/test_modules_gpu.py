"""Every module of the Keras hybrid alone against fp64, at the benchmark's shapes.

The library's module probe (ishara_debug_module_forward / _backward / ishara_debug_head_loss_backward) runs one module through the model's
own orchestration, so the fused training kernels the benchmark times are what is compared: the A-stationary GEMM with its LayerNorm /
per-sample-affine prologue and side outputs, the training epilogues (pre_out, dropout, rowscale, addtab, dact, QKV scatter), the weight
gradient variants (per-sample-affine, bias_rowscale, padded operands, deferred slab sums), the fused depthwise / BatchNorm backward, the
ECA / SE / BatchNorm finalize kernels and the deferred reductions.  Per case: y, dx, every parameter gradient of the module, the implied
BatchNorm batch statistics, exact zeros in every other gradient entry, intact workspace guards — once as the product runs the module and
once under the profiler (non-deferred weight-gradient form), whose report names the kernels the case is meant to reach.

Metrics and bounds: tests/module_parity.py (f32: the operator tests' bounds; bf16: 2x observed per module kind, at most 0.03 rel-L2;
tests/test_module_mutants.py shows the bf16 bounds reject ordinary mistakes).  Observed values are logged through test_model_gpu._log_observed (the parity log DESIGN.md §2 quotes)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import module_parity as MP
from ishara_amd import _lib, get_model
from oracle import ishara_oracle as O
from test_model_gpu import _log_observed

pytestmark = pytest.mark.gpu

SHAPES = {
    # configs[1] of the benchmark: d256, T384, F224, 8 heads, kernel sizes 11 / 5 / 3, transformer kernel 15 (one block of each kind: the modules
    # of the second block have the same shapes)
    "cfg2": dict(dim=256, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, kernel_sizes=[11, 5, 3], num_conv_per_block=3, num_heads=8,
                 expansion_factor=2, transformer_kernel_size=15, input_shape=(384, 224)),
    # the d512 / T512 model of test_full_size_gpu.py
    "d512": dict(dim=512, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, kernel_sizes=[11, 5, 3], num_conv_per_block=3, num_heads=8,
                 expansion_factor=2, transformer_kernel_size=15, input_shape=(512, 224)),
}
ALL = ["stem", "convsqueeze_0_1", "convsqueeze_0_2", "convsqueeze_0_3", "squeezeformer_0/ffn1", "squeezeformer_0/mha", "squeezeformer_0/conv",
       "conformer_0/ffn1", "conformer_0/mha", "conformer_0/conv", "conformer_0/ffn2", "head"]
NO_ATTN = [n for n in ALL if not n.endswith("/mha")]
PSA_KEY = "gemm_tn_tr_kernel<0,false,true>"
B_NO_PSA = 11      # a prime above 8: no split of whole samples with at most 8 per split (gemm_tn_psa_ok refuses it); M = 4224 is still a multiple of 64


def _cases():
    out = []

    def add(shape, dtype, dropout, B, names, variant=""):
        out.extend((shape, dtype, dropout, B, variant, n) for n in names)

    for dtype in ("f32", "bf16"):
        for dropout in (0.0, 0.2):
            add("cfg2", dtype, dropout, 2, ALL)                       # one sample per PSA split
    for dropout in (0.0, 0.2):                                         # two samples per PSA split, M = 24576 (attention: with dropout only, to bound the run time)
        add("cfg2", "bf16", dropout, 64, ALL if dropout > 0 else NO_ATTN)
        add("cfg2", "bf16", dropout, B_NO_PSA, ["convsqueeze_0_1"])
    add("cfg2", "f32", 0.2, 64, NO_ATTN)
    for dropout in (0.0, 0.2):
        add("d512", "bf16", dropout, 16, ALL if dropout > 0 else NO_ATTN)
    add("d512", "f32", 0.2, 16, ["convsqueeze_0_1", "squeezeformer_0/ffn1", "head"])
    add("d512", "bf16", 0.2, 64, NO_ATTN)                              # M = 32768: the big-tile GEMMs, the four-chunk ECA finalize (c = 1024)
    add("d512", "bf16", 0.0, 64, ["convsqueeze_0_1"])
    for variant in ("no_psa", "no_deferred_reduce", "no_deferred_slab_sums", "regstage8192", "regstage4"):
        add("cfg2", "bf16", 0.2, 64, ["convsqueeze_0_1", "squeezeformer_0/ffn1"], variant)
    return out


VARIANT_ENV = {"no_psa": "ISHARA_NO_PSA", "no_deferred_reduce": "ISHARA_NO_DEFERRED_REDUCE", "no_deferred_slab_sums": "ISHARA_NO_DEFERRED_SLAB_SUMS"}
_cache = {}


def _kw(shape):
    """the model fields of a shape: a name in SHAPES, or the dict itself (tests/test_modules_ragged_gpu.py)"""
    return SHAPES[shape] if isinstance(shape, str) else shape


def _model(shape, dtype, dropout, B, variant):
    """One model per (shape, dtype, dropout, B, create-time switch), kept until the next key asks (cases are ordered by key)."""
    key = (repr(shape), dtype, dropout, B, VARIANT_ENV.get(variant, ""))
    if _cache.get("key") != key:
        _cache.clear()
        torch.cuda.empty_cache()
        env = VARIANT_ENV.get(variant)
        os.environ["ISHARA_WS_GUARD"] = "1"       # both read at ishara_create
        if env:
            os.environ[env] = "1"
        try:
            model = get_model(**_kw(shape), dropout_rate=dropout, head_dropout=0.4 if dropout > 0 else 0.0,
                              conformer_attn_dropout=0.1 if dropout > 0 else 0.0, dtype=dtype, max_batch=B, seed=3)
        finally:
            os.environ.pop("ISHARA_WS_GUARD", None)
            if env:
                os.environ.pop(env, None)
        W = MP.perturbed(model.get_weights(), dtype)
        model.set_weights(W)
        _cache.update(key=key, model=model, W=W, flat=model.params.clone())
    return _cache["model"], _cache["W"], _cache["flat"]


def _ocfg(shape, dropout):
    kw = dict(_kw(shape))
    kw["kernel_sizes"] = tuple(kw["kernel_sizes"])
    return O.Config(dropout_rate=dropout, head_dropout=0.4 if dropout > 0 else 0.0, conformer_attn_dropout=0.1 if dropout > 0 else 0.0, **kw)


def _report(model):
    buf = C.create_string_buffer(1 << 16)
    n = model._lib.ishara_profile_report(model._h, buf, len(buf))
    assert n >= 0, model._lib.ishara_last_error()
    return [line.split()[0] for line in buf.value.decode().splitlines()]


def _check_routes(name, kind, shape, dtype, dropout, B, variant, report):
    """the kernels the case is meant to reach, by their names in the profile report"""
    if dtype != "bf16":
        return
    pro = MP.prologue_kinds(report)
    plain = variant in ("", "no_deferred_reduce", "no_deferred_slab_sums")
    if kind == "conv":
        if plain or variant == "no_psa":
            assert 2 in pro, f"no A-stationary GEMM with the per-sample-affine prologue in {report}"
            assert "dwconv_bwd" in report and "bn_bwd_apply" not in report, f"not the fused depthwise / BatchNorm backward: {report}"
        if plain and B != B_NO_PSA:
            assert PSA_KEY in report, f"the project conv's weight gradient did not take the per-sample-affine route: {report}"
            assert "sample_affine" not in report and "sample_reduce" not in report
        if B == B_NO_PSA or variant == "no_psa":
            assert PSA_KEY not in report, f"the per-sample-affine route was not refused: {report}"
            assert "sample_reduce" in report
        if shape in SHAPES:      # the profiled keys agree with what the plan says for the case (the forced switches of a variant are set while this runs)
            kw = SHAPES[shape]
            flags = (1 if dropout > 0 else 0) | (0 if variant == "no_psa" else 4)
            plan = _lib.load().ishara_debug_conv_block_route_name(1, 1, B, kw["input_shape"][0], kw["dim"], kw["kernel_sizes"][int(name[-1]) - 1], flags).decode()
            fwd, bwd = plan.split("|")
            assert ("+psa" in fwd) == (PSA_KEY in report) == ("sample_reduce" not in report), (plan, report)
            assert ("+affine" in fwd) == ("sample_affine" in report) and ("+prologue" in fwd) == (2 in pro), (plan, report)
            assert bwd.endswith("fused_bn") == ("bn_bwd_apply" not in report) and ("scaled_copy" in bwd) == ("map_rows" in report), (plan, report)
    if (kind in ("ffn", "sqzconv") or (kind == "mha" and shape == "cfg2")) and plain:      # (d512: the K = 512 QKV projection runs the LayerNorm kernel and a tile GEMM)
        assert 1 in pro, f"no A-stationary GEMM with the LayerNorm prologue in {report}"
    if variant == "regstage8192":
        assert not pro and not any(k.startswith("gemm_nt_as") for k in report), report
    if shape == "d512" and B == 64 and kind in ("conv", "ffn"):
        assert "gemm_tn_big_kernel" in report, f"no big-tile weight-gradient GEMM at M = 32768: {report}"
        assert "gemm_nt_big_kernel<bf16>" in report, f"no big-tile NT GEMM at M = 32768: {report}"


@pytest.mark.parametrize("shape,dtype,dropout,B,variant,name", _cases(),
                         ids=lambda v: str(v).replace("/", ".") if not isinstance(v, float) else f"drop{v}")
def test_module_matches_fp64(shape, dtype, dropout, B, variant, name):
    check_module(shape, dtype, dropout, B, variant, name)


def check_module(shape, dtype, dropout, B, variant, name, kw=None, log_test="module", check_routes=_check_routes):
    """One module at one case against fp64, product route and profiled route.  kw: the model fields where `shape` is only the case's label
    (tests/test_modules_ragged_gpu.py); check_routes(name, kind, shape, dtype, dropout, B, variant, report): what the profile report must name."""
    if kw is None:
        kw = shape
    model, W, flat = _model(kw, dtype, dropout, B, variant)
    lib = model._lib
    ocfg = _ocfg(kw, dropout)
    names = model.module_names()
    assert names == MP.expected_modules(ocfg)
    i = names.index(name)
    _, cin, cout, first, nsites = model._module_info(i)
    kind = MP.module_kind(name)
    T = ocfg.T
    g = np.random.default_rng(1000 + i)
    x = MP.round_to(g.standard_normal((B, T, cin)), dtype)
    seed = 4242
    if kind == "conv" and dropout > 0:
        seed = MP.mixed_droppath_seed(seed, first, B, dropout)
        keep = MP.rng.keep_mask(seed, first, B, 1, dropout)[:, 0]
        assert keep.any() and not keep.all()
    labels = dy = None
    if kind == "head":
        _, labels = O.synthetic_batch(ocfg, B, seed=2)
    else:
        dy = MP.round_to(g.standard_normal((B, T, cout)), dtype)
    ref = MP.reference(name, ocfg, W, x, dy, seed, first, labels=labels)
    assert ref["sites_used"] == nsites
    bound = MP.bounds(kind, dtype, shape)
    mine = np.zeros(model.n_train, bool)
    for n, s, o, t in model.entries:
        if t and MP.owns(name, n):
            mine[o:o + int(np.prod(s))] = True
    regstage = {"regstage8192": 8192, "regstage4": 4}.get(variant, 0)
    failures = []
    try:
        if regstage:
            lib.ishara_debug_force_regstage(regstage)
        for route in ("product", "profiled"):
            model.params.copy_(flat)          # the training forward updates the moving statistics in place
            if route == "profiled":
                _lib.check(lib.ishara_profile_enable(model._h, 1))
            try:
                y = model.module_forward(i, x, training=True, seed=seed)
                if kind == "head":
                    dx = model.module_backward(i, y, labels=labels)
                else:
                    dx = model.module_backward(i, dy)
                torch.cuda.synchronize()
                report = _report(model) if route == "profiled" else None
            finally:
                if route == "profiled":
                    lib.ishara_profile_enable(model._h, 0)
            _lib.check(lib.ishara_workspace_guard_check(model._h), "workspace guard (a kernel wrote outside its buffer)")
            gflat = model.grads[:model.n_train].cpu().numpy()
            pflat = model.params.cpu().numpy()
            got = dict(y=y.cpu().numpy(), dx=None if dx is None else dx.cpu().numpy(),
                       grads={n: gflat[o:o + int(np.prod(s))].reshape(s) for n, s, o, t in model.entries if t and MP.owns(name, n)},
                       stats={n: pflat[o:o + int(np.prod(s))].reshape(s) for n, s, o, t in model.entries if not t and MP.owns(name, n)},
                       loss=float(model._loss_buf.item()) if kind == "head" else None)
            assert np.isfinite(got["y"]).all() and np.isfinite(gflat).all()
            stray = int(np.count_nonzero(gflat[~mine]))
            assert stray == 0, f"{stray} gradient elements outside {name}'s entries are not zero"
            assert np.array_equal(pflat[:model.n_train], flat[:model.n_train].cpu().numpy()), "a module run changed trainable parameters"
            obs, bad = MP.compare(name, dtype, B, T, got, ref, W, bound)
            _log_observed(dict(test=log_test, module=name, kind=kind, shape=shape, dtype=dtype, dropout=dropout, B=B, variant=variant, route=route, **obs))
            print(f"observed[{route}] {obs}")
            failures += [f"[{route}] {b}" for b in bad]
            if report is not None:
                check_routes(name, kind, shape, dtype, dropout, B, variant, report)
    finally:
        if regstage:
            lib.ishara_debug_force_regstage(0)
        model.params.copy_(flat)
    assert not failures, "\n".join(failures)


def test_probe_refusals_on_a_bound_handle():
    """a backward without the matching training forward, the head through module_backward, the stem with a dx, and ishara_loss_backward after a
    probe forward are refused; a refused call launches nothing (the gradients stay as they were)"""
    model, W, flat = _model("cfg2", "f32", 0.0, 2, "")
    lib = model._lib
    names = model.module_names()
    i = names.index("squeezeformer_0/ffn1")
    x = torch.zeros((2, 384, 256), device=model.device)
    model.grads.fill_(7.0)
    model.module_forward(i, x, training=False)
    for call, word in [(lambda: model.module_backward(i, x), "training=1"),
                       (lambda: model.module_backward(i + 1, x), "training=1")]:
        with pytest.raises(_lib.IsharaError, match=word):
            call()
    model.module_forward(i, x, training=True, seed=1)
    with pytest.raises(_lib.IsharaError, match="training=1"):
        model.module_backward(i, x[:1])                           # another batch size
    with pytest.raises(_lib.IsharaError, match="ishara_forward"):
        y = torch.full((2, 64), 59, dtype=torch.int64)
        _lib.check(lib.ishara_loss_backward(model._h, _lib.ptr(torch.zeros((2, 384, 60), device=model.device)), _lib.ptr(y.to(model.device)), 2, None, None,
                                            C.c_float(1.0), _lib.stream()), "ishara_loss_backward")
    h = len(names) - 1
    logits = model.module_forward(h, x, training=True, seed=1)
    with pytest.raises(_lib.IsharaError, match="ishara_debug_head_loss_backward"):
        model.module_backward(h, logits)
    torch.cuda.synchronize()
    assert bool((model.grads == 7.0).all())
    model.grads.zero_()
