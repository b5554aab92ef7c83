"""CPU: the host side of minimum-risk training (ishara_amd/mwer.py): mwer_reference's analytic gradient against central differences of the
fp64 risk, the properties of the risk and its coefficients, the closed form of a hypothesis with exactly one alignment, the case tables of
tests/mwer_parity.py under their own twins, the Optimizer's mwer_* options, the optional key of the state file, the new symbols of the
header, and the refusals of the C entry points (made-up addresses: a refused call dereferences nothing)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mwer_parity as P
import rescore_parity as RP
from ishara_amd import mwer, rescore, train_state as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ = None
A = lambda a: C.c_void_p(a)      # noqa: E731  made-up addresses


# ---------------------------------------------------------------------------------- the definition
def _small():
    g = np.random.default_rng(77)
    x = g.standard_normal((6, 4)) * 1.5
    hyps = [[0, 1], [2], [1, 1, 0]]
    return x, hyps, [0, 2, 1]


@pytest.mark.parametrize("inv_temp, normalise", [(1.0, True), (0.5, False), (2.5, True)])
def test_analytic_gradient_equals_central_differences_of_the_fp64_risk(inv_temp, normalise):
    x, hyps, tgt = _small()                                  # T 6, C 4, N 3, blank 3
    ref = mwer.mwer_reference(x, hyps, tgt, 3, inv_temp, normalise)
    assert np.isclose(ref["risk"], mwer.risk_of(x, hyps, tgt, 3, inv_temp, normalise), rtol=1e-12)
    h = 1e-5
    num = np.zeros_like(x)
    for t in range(x.shape[0]):
        for k in range(x.shape[1]):
            d = np.zeros_like(x)
            d[t, k] = h
            num[t, k] = (mwer.risk_of(x + d, hyps, tgt, 3, inv_temp, normalise) - mwer.risk_of(x - d, hyps, tgt, 3, inv_temp, normalise)) / (2 * h)
    assert np.abs(ref["grad"]).max() > 1e-3
    assert np.allclose(ref["grad"], num, rtol=1e-6, atol=1e-6 * np.abs(num).max()), np.abs(ref["grad"] - num).max()


def test_posterior_reference_agrees_with_the_forward_algorithm_and_sums_to_one():
    g = np.random.default_rng(78)
    x = g.standard_normal((9, 5)) * 2
    for h in ([], [1], [0, 0, 2], [3, 1, 3, 3]):
        logp, post = mwer.ctc_posterior_reference(x, h, 4)
        assert np.isclose(logp, rescore.ctc_logp_reference(x, h, 4), rtol=1e-12)
        assert np.allclose(post.sum(axis=1), 1.0, atol=1e-12)
    logp, post = mwer.ctc_posterior_reference(x[:3], [0, 0, 1], 4)      # 3 + 1 > 3 frames
    assert logp == -np.inf and not post.any()


def test_coefficients_sum_to_zero_and_the_risk_lies_between_the_distances():
    g = np.random.default_rng(79)
    for trial in range(20):
        N = int(g.integers(1, 9))
        logp = -np.abs(g.standard_normal(N)) * 5
        logp[g.random(N) < 0.2] = -np.inf
        dist = g.integers(0, 12, N)
        W, post, risk, coef = mwer.risk_reference(logp, dist, 7, float(g.uniform(0.2, 3)), bool(trial % 2))
        live = np.isfinite(logp)
        if not live.any():
            assert np.isnan(risk) and not coef.any() and not post.any()
            continue
        assert abs(coef.sum()) <= 1e-12 * max(np.abs(coef).sum(), 1e-300) + 1e-15
        assert W[live].min() - 1e-12 <= risk <= W[live].max() + 1e-12
        assert np.isclose(post.sum(), 1.0) and not coef[~live].any()


def test_one_alignment_has_the_closed_form_softmax_minus_onehot():
    case = next(c for c in P.grad_cases() if c["name"] == "tight")
    tb = RP.clip_frames(case, 0)
    x = case["logits"][0, :tb].astype(np.float64)
    sm = np.exp(mwer._log_softmax(x))
    for n, path_syms in ((0, None), (1, None), (2, None)):
        h = P.hyp_of(case, 0, n)
        assert len(h) + RP.repeats_of(h) == tb                # exactly one alignment: symbol, blank between repeats
        path = []
        for i, c in enumerate(h):
            if i > 0 and h[i - 1] == c:
                path.append(case["blank"])
            path.append(c)
        onehot = np.zeros_like(x)
        onehot[np.arange(tb), path] = 1.0
        coef = np.zeros(case["N"])
        coef[n] = 1.0
        G, _, logp = mwer.nbest_grad_reference(x, [P.hyp_of(case, 0, k) if k == n else None for k in range(case["N"])], coef, case["blank"])
        assert np.allclose(G, sm - onehot, atol=1e-12)
        assert np.isclose(logp[n], np.log(sm[np.arange(tb), path]).sum())


def test_case_tables_hold_under_their_own_twins():
    assert {0, 1, 31, 32, 33, 63, 64, 127, 128, 255} <= {int(v) for c in P.grad_cases() for v in c["hyp_len"].ravel()}
    assert {c["T"] for c in P.grad_cases()} >= {1, 7, 8, 9, 17, 33, 272} and {c["N"] for c in P.grad_cases()} >= {1, 3, 4, 5, 64}
    assert {(c["C"], c["blank"]) for c in P.grad_cases()} >= {(2, 1), (8, 7), (60, 59), (64, 0)}
    for case in P.grad_cases():
        assert case["B"] <= 4 and (case["T"] <= 64 or case["name"] == "seams-272")
        fails, ratio = P.check_grad(case, P.twin_grad(case).astype(np.float32))
        assert not fails and ratio < 0.01, (case["name"], fails, ratio)
    st = np.concatenate([P.expected_status(c).ravel() for c in P.grad_cases()])
    assert {0, 1, 2, 4, 8} <= set(st.tolist())
    for case in P.weight_cases():
        fails, _ = P.check_weights(case, P.twin_weights(case))
        assert not fails, (case["name"], fails)
    assert any(not P.live_of(c).any(axis=1).all() for c in P.weight_cases())      # a clip with no live slot


def test_weights_twin_agrees_with_the_definition():
    for case in P.weight_cases():
        tw = P.twin_weights(case)
        live = P.live_of(case)
        for b in range(case["B"]):
            lp = np.where(live[b], case["logp"][b].astype(np.float64), -np.inf)
            hyps = [case["hyp_idx"][b, n, :case["hyp_len"][b, n]].tolist() if live[b, n] else None for n in range(case["N"])]
            dist = [mwer.levenshtein(h, rescore.target_symbols(case["targets"][b])) if h is not None else -1 for h in hyps]
            it = 1.0 if case["inv_temp"] is None else float(case["inv_temp"])
            _, post, risk, coef = mwer.risk_reference(lp, dist, int(tw["tlen"][b]), it, case["mode"] == 1)
            assert np.array_equal(np.asarray(dist), tw["dist"][b])
            if live[b].any():
                assert np.allclose(tw["risk"][b], risk, rtol=1e-5) and np.allclose(tw["coef"][b], coef, rtol=1e-4, atol=1e-6)
            else:
                assert np.isnan(tw["risk"][b]) and np.isnan(risk)


# ---------------------------------------------------------------------------------- Optimizer / Model without a device
def test_optimizer_mwer_options_are_checked():
    from ishara_amd import Optimizer
    assert Optimizer().mwer_options() == dict(mwer_nbest=0, mwer_beam_width=8, mwer_weight=1.0, mwer_ctc_weight=0.01, mwer_temperature=1.0,
                                              mwer_normalise=True, mwer_start_step=0)
    assert tuple(Optimizer().mwer_options()) == mwer.OPTION_NAMES and len(mwer.OPTION_NAMES) == 7
    assert Optimizer().awp_options() == (None, 1e-4, 0, False) and Optimizer().train_options() == (1, 0.0, False)      # the existing tuples are what they were
    o = Optimizer(mwer_nbest=4, mwer_beam_width=16, mwer_weight=0.5, mwer_ctc_weight=0, mwer_temperature=2, mwer_normalise=False, mwer_start_step=np.int64(300))
    assert o.mwer_options() == dict(mwer_nbest=4, mwer_beam_width=16, mwer_weight=0.5, mwer_ctc_weight=0.0, mwer_temperature=2.0, mwer_normalise=False,
                                    mwer_start_step=300)
    for bad in (dict(mwer_nbest=-1), dict(mwer_nbest=65), dict(mwer_nbest=2.0), dict(mwer_nbest=True), dict(mwer_nbest=None), dict(mwer_nbest=9),
                dict(mwer_beam_width=0), dict(mwer_beam_width=33), dict(mwer_beam_width="8"),
                dict(mwer_weight=-1.0), dict(mwer_weight=float("nan")), dict(mwer_weight=float("inf")), dict(mwer_weight=None), dict(mwer_weight=True),
                dict(mwer_ctc_weight=-0.01), dict(mwer_ctc_weight="0.01"),
                dict(mwer_temperature=0.0), dict(mwer_temperature=-1.0), dict(mwer_temperature=float("inf")), dict(mwer_temperature=None),
                dict(mwer_normalise=1), dict(mwer_normalise=None),
                dict(mwer_start_step=-1), dict(mwer_start_step=2.0), dict(mwer_start_step=True)):
        with pytest.raises(ValueError, match="mwer_"):
            Optimizer(**dict(dict(mwer_nbest=4), **bad)).mwer_options()
    with pytest.raises(ValueError, match="mwer_temperature"):
        Optimizer(mwer_temperature=0.0).mwer_options()       # checked also while mwer_nbest is 0


def test_model_without_such_a_step_allocates_nothing_and_refuses_its_reader():
    from ishara_amd import Optimizer, _lib, make_config
    from ishara_amd.model import Model
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4), device=None)
    assert m._mwer is None and m._mwer_begin_step(4) is None
    m.compile(optimizer=Optimizer(mwer_nbest=4, mwer_start_step=5))
    assert m._mwer_begin_step(4) is None and m._mwer is None                 # not started yet: nothing is allocated
    with pytest.raises(_lib.IsharaError, match="no step has run with minimum-risk training"):
        m.mwer_stats()
    m.optimizer.mwer_weight = -1.0                              # the options are plain attributes, checked when a step reads them
    with pytest.raises(ValueError, match="mwer_weight"):
        m._mwer_begin_step(4)


# ---------------------------------------------------------------------------------- the state file
ENTRIES = [("stem/kernel", (6, 4), 0, True), ("stem/bias", (4,), 24, True), ("bn/moving_mean", (4,), 28, False), ("bn/moving_variance", (4,), 32, False)]
OPTS = dict(mwer_nbest=4, mwer_beam_width=16, mwer_weight=0.5, mwer_ctc_weight=0.02, mwer_temperature=2.0, mwer_normalise=False, mwer_start_step=300)


def _state(**kw):
    g = np.random.default_rng(9)
    args = dict(iterations=7, steps=7, step_seed=23774, learning_rate=4e-3, weight_decay=2e-4, apply_weight_decay=True, global_clipnorm=1.5,
                skip_nonfinite=True, accumulate_steps=2, skipped=1)
    args.update(kw)
    return TS.pack_state(ENTRIES, g.standard_normal(36).astype(np.float32), *(g.standard_normal(28).astype(np.float32) for _ in range(3)), **args)


def test_state_without_mwer_has_exactly_the_old_keys():
    assert set(_state()) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS) and TS.FORMAT_VERSION == 1
    assert "mwer" not in TS.unpack_state(_state(), ENTRIES) and TS.MWER_KEYS == ("mwer",)


def test_state_with_mwer_round_trips_as_one_key(tmp_path):
    st = _state(mwer=OPTS)
    assert set(st) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.MWER_KEYS)
    np.savez(str(tmp_path / "run.npz"), **st)
    with np.load(str(tmp_path / "run.npz"), allow_pickle=False) as z:
        back = TS.unpack_state(z, ENTRIES)
    assert back["mwer"] == OPTS
    for k in TS.ARRAYS:
        assert back[k].tobytes() == st[k].tobytes()
    both = _state(mwer=OPTS, awp_delta=0.5, ema_avg=np.zeros(28, np.float32))
    assert set(both) == set(TS.ARRAYS + TS.SCALARS + TS.ENTRY_KEYS + TS.EMA_KEYS + TS.AWP_KEYS + TS.MWER_KEYS)


def test_state_refuses_wrong_mwer_options():
    good = _state(mwer=OPTS)
    for text in ('{"mwer_nbest": -1}', '{"mwer_nbest": 4, "mwer_depth": 2}', "[4]", '{"mwer_temperature": 0}'):
        with pytest.raises(TS.TrainStateError, match="'mwer'"):
            TS.unpack_state(dict(good, mwer=np.array(text, dtype=np.str_)), ENTRIES)
    with pytest.raises(ValueError, match="mwer_nbest"):
        _state(mwer=dict(OPTS, mwer_nbest=99))


# ---------------------------------------------------------------------------------- the header and the C entry points
def test_new_symbols_are_declared_in_the_header_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    for name in ("ishara_ctc_nbest_grad_workspace_bytes", "ishara_ctc_nbest_grad", "ishara_mwer_weights", "ishara_loss_backward_nbest"):
        assert re.search(r"\b(int|int64_t) " + name + r"\(", hdr), name
        assert hasattr(lib, name), name
    import ishara_amd
    for name in ("ctc_nbest_grad", "mwer_weights", "mwer_reference", "mwer_loss"):
        assert callable(getattr(ishara_amd, name))


def test_sources_keep_the_launch_conditions():
    for f in ("ctc_nbest_grad.hip", "mwer_weights.hip"):
        src = open(os.path.join(ROOT, "ishara_amd", "csrc", f)).read()
        code = "\n".join(line.split("//")[0] for line in src.splitlines())
        assert "hipMalloc" not in code and "hipMemset" not in code and "Synchronize" not in code and "hipMemcpy" not in code, f
        for m in re.finditer(r"atomicAdd\(&(\w+)", code):
            assert m.group(1) == "cls", f"{f}: an atomic that is not the LDS scatter-add"


def test_workspace_bytes(lib):
    ws = lib.ishara_ctc_nbest_grad_workspace_bytes
    for B, T, N, ml in ((1, 1, 1, 1), (2, 16, 3, 31), (2, 16, 3, 32), (64, 384, 4, 64), (256, 384, 8, 64), (3, 272, 4, 255)):
        rows = 64 * ((2 * ml + 1 + 63) // 64)
        assert ws(B, T, N, ml) == (B * N * 12 + 15) // 16 * 16 + 16 * B * N * T * rows, (B, T, N, ml)
    assert 2.4e9 < ws(256, 384, 8, 64) < 2.5e9               # the figure of DESIGN.md §4: sized by max_len, not by Th = T
    assert ws(0, 16, 3, 31) == 0
    for B, T, N, ml in ((-1, 16, 3, 31), (65536, 16, 3, 31), (2, 0, 3, 31), (2, 4097, 3, 31), (2, 16, 0, 31), (2, 16, 65, 31), (2, 16, 3, 0), (2, 16, 3, 256)):
        assert ws(B, T, N, ml) == -1, (B, T, N, ml)


def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), f"{name}: the error is not the entry point's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


def test_nbest_grad_refusals(lib):
    name = "ishara_ctc_nbest_grad"
    P0 = dict(logits=1 << 20, hyp_idx=2 << 20, hyp_len=3 << 20, coef=4 << 20, dlogits=5 << 20, ws=6 << 20)

    def call(B=2, T=16, Cn=8, blank=7, N=3, Th=16, max_len=16, accumulate=0, frame_len=N_, dlb=N_, logp=N_, status=N_, **ptr):
        a = {k: A(v) for k, v in P0.items()}
        a.update(ptr)
        return lib.ishara_ctc_nbest_grad(a["logits"], B, T, Cn, blank, a["hyp_idx"], a["hyp_len"], N, Th, max_len, frame_len, a["coef"], C.c_float(1.0),
                                         a["dlogits"], accumulate, dlb, logp, status, a["ws"], N_)
    for kw, word in ((dict(Cn=1), "C=1"), (dict(Cn=65), "C=65"), (dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(Th=0), "Th=0"), (dict(Th=4097), "Th=4097"),
                     (dict(N=0), "N=0"), (dict(N=65), "N=65"), (dict(max_len=0), "max_len=0"), (dict(max_len=256), "max_len=256"), (dict(B=-1), "B=-1"),
                     (dict(B=65536), "B=65536"), (dict(blank=8), "blank 8"), (dict(accumulate=2), "accumulate=2")):
        _refused(lib, call(**kw), name, word)
    for k in P0:
        _refused(lib, call(**{k: N_}), name, "null")
    for k in ("logits", "hyp_idx", "hyp_len", "coef", "dlogits"):
        _refused(lib, call(**{k: A(P0[k] + 2)}), name, "misaligned")
    for k in ("frame_len", "dlb", "logp", "status"):
        _refused(lib, call(**{k: A((7 << 20) + 1)}), name, "misaligned")
    _refused(lib, call(ws=A(P0["ws"] + 8)), name, "misaligned workspace", "16-byte")
    _refused(lib, call(dlogits=A(P0["logits"])), name, "dlogits overlaps logits")
    _refused(lib, call(dlogits=A(P0["logits"] + 2 * 16 * 8 * 4 - 4)), name, "overlaps")
    assert call(B=0) == 0                                    # a no-op: nothing is launched, nothing is dereferenced


def test_mwer_weights_refusals(lib):
    name = "ishara_mwer_weights"
    P0 = dict(hyp_idx=1 << 20, hyp_len=2 << 20, logp=3 << 20, targets=4 << 20, dist=5 << 20, post=6 << 20, risk=7 << 20, coef=8 << 20, tlen=9 << 20)

    def call(B=2, N=3, Th=16, L=12, mode=1, status=N_, inv_temp=N_, **ptr):
        a = {k: A(v) for k, v in P0.items()}
        a.update(ptr)
        return lib.ishara_mwer_weights(a["hyp_idx"], a["hyp_len"], a["logp"], status, B, N, Th, a["targets"], L, inv_temp, mode, a["dist"], a["post"],
                                       a["risk"], a["coef"], a["tlen"], N_)
    for kw, word in ((dict(N=0), "N=0"), (dict(N=65), "N=65"), (dict(Th=0), "Th=0"), (dict(Th=4097), "Th=4097"), (dict(L=0), "L=0"), (dict(L=65), "L=65"),
                     (dict(mode=2), "mode 2"), (dict(mode=-1), "mode -1"), (dict(B=-1), "B=-1")):
        _refused(lib, call(**kw), name, word)
    for k in P0:
        _refused(lib, call(**{k: N_}), name, "null")
        _refused(lib, call(**{k: A(P0[k] + 1)}), name, "misaligned")
    for k in ("status", "inv_temp"):
        _refused(lib, call(**{k: A((10 << 20) + 2)}), name, "misaligned")
    assert call(B=0) == 0


def test_loss_backward_nbest_refuses_before_any_launch(lib):
    name = "ishara_loss_backward_nbest"
    rc = lib.ishara_loss_backward_nbest(N_, A(1 << 20), A(2 << 20), 2, N_, N_, C.c_float(1.0), N_, A(3 << 20), A(4 << 20), 3, 16, 16, A(5 << 20), C.c_float(1.0),
                                        A(6 << 20), N_)
    _refused(lib, rc, name, "null model")
