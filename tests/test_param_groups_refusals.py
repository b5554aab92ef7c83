"""CPU: the library loads without a GPU, and the five entry points of the optimizer's parameter groups refuse, by their own message and
before any HIP call (made-up addresses: a refused call dereferences nothing): null pointers, buffers off a 16-byte boundary, seg_off or ws
off an 8-byte and groups or st off a 4-byte boundary, n outside 1 .. 2^31 - 1, S outside 1 .. n, iteration < 1, the skip switch without
a record."""
import ctypes as C

import pytest

N = None
P = lambda a: C.c_void_p(a)      # noqa: E731  made-up addresses
F = C.c_float
BUFS = dict(theta=1 << 20, grad=2 << 20, m=3 << 20, v=4 << 20, slow=5 << 20)
TABLE = dict(seg_off=6 << 20, groups=7 << 20, ws=8 << 20)
ST = 9 << 20


def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), f"{name}: the error is not the entry point's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


def test_the_library_loads_without_a_gpu(lib):
    for name in ("ishara_param_groups_workspace_bytes", "ishara_optimizer_step_groups", "ishara_gradient_mask_groups", "ishara_optimizer_op_step",
                 "ishara_optimizer_op_step_groups"):
        assert hasattr(lib, name), name


def test_workspace_bytes(lib):
    ws = lib.ishara_param_groups_workspace_bytes
    for n, S in ((1, 1), (5, 1), (4097, 3), (10 ** 6, 107), (2 ** 31 - 1, 1000)):
        assert ws(n, S) == 8 * (S + 1), (n, S)
    for n, S in ((0, 1), (-1, 1), (2 ** 31, 1), (5, 0), (5, 6), (5, -1)):
        assert ws(n, S) == -1 and (lib.ishara_last_error() or b"").decode().startswith("ishara_param_groups_workspace_bytes:"), (n, S)


def _op(lib, grouped):
    def call(n=100, iteration=1, st=P(ST), skip=0, S=7, **ptrs):
        a = {k: P(v) for k, v in dict(BUFS, **TABLE).items()}
        a.update(ptrs)
        head = (a["theta"], a["grad"], a["m"], a["v"], a["slow"], n, iteration, F(4e-3), F(0.01), st, skip)
        if grouped:
            return lib.ishara_optimizer_op_step_groups(*head, a["seg_off"], a["groups"], S, a["ws"], N)
        return lib.ishara_optimizer_op_step(*head, N)
    return call


@pytest.mark.parametrize("grouped", [False, True])
def test_operator_refusals(lib, grouped):
    name = "ishara_optimizer_op_step_groups" if grouped else "ishara_optimizer_op_step"
    call = _op(lib, grouped)
    for k, a in BUFS.items():
        _refused(lib, call(**{k: N}), name, f"null {k}")
        for off in (4, 8, 12):
            _refused(lib, call(**{k: P(a + off)}), name, f"misaligned {k}", "16-byte")
    for n in (0, -1, 2 ** 31, 2 ** 40):
        _refused(lib, call(n=n), name, f"n={n}", "1..2147483647")
    for it in (0, -1, -2 ** 31):
        _refused(lib, call(iteration=it), name, f"iteration={it}")
    _refused(lib, call(st=P(ST + 2)), name, "misaligned st", "4-byte")
    _refused(lib, call(st=N, skip=1), name, "skip_nonfinite needs the record", "null st")
    if not grouped:
        return
    for k, a in TABLE.items():
        _refused(lib, call(**{k: N}), name, f"null {k}")
    _refused(lib, call(seg_off=P(TABLE["seg_off"] + 4)), name, "misaligned seg_off", "8-byte")
    _refused(lib, call(ws=P(TABLE["ws"] + 4)), name, "misaligned ws", "8-byte")
    _refused(lib, call(groups=P(TABLE["groups"] + 2)), name, "misaligned groups", "4-byte")
    for S in (0, -1, 101):
        _refused(lib, call(S=S), name, f"S={S}", "1..n=100")


def test_mask_refusals(lib):
    name = "ishara_gradient_mask_groups"

    def call(g=P(BUFS["grad"]), n=100, S=7, **ptrs):
        a = {k: P(v) for k, v in TABLE.items()}
        a.update(ptrs)
        return lib.ishara_gradient_mask_groups(N, g, n, a["seg_off"], a["groups"], S, a["ws"], N)

    _refused(lib, call(g=N), name, "null g")
    for off in (4, 8, 12):
        _refused(lib, call(g=P(BUFS["grad"] + off)), name, "misaligned g", "16-byte")
    for k in TABLE:
        _refused(lib, call(**{k: N}), name, f"null {k}")
    _refused(lib, call(seg_off=P(TABLE["seg_off"] + 4)), name, "misaligned seg_off", "8-byte")
    _refused(lib, call(ws=P(TABLE["ws"] + 4)), name, "misaligned ws", "8-byte")
    _refused(lib, call(groups=P(TABLE["groups"] + 2)), name, "misaligned groups", "4-byte")
    for n in (0, -1, 2 ** 31):
        _refused(lib, call(n=n), name, f"n={n}", "1..2147483647")
    for S in (0, -1, 101):
        _refused(lib, call(S=S), name, f"S={S}", "1..n=100")


def test_model_step_refusals(lib):
    """the handle is checked first; what follows it is checked before the handle is read (a made-up handle is never dereferenced)"""
    name = "ishara_optimizer_step_groups"
    H = P(10 << 20)

    def call(h=H, grad=N, st=N, skip=0, S=7, **ptrs):
        a = {k: P(v) for k, v in TABLE.items()}
        a.update(ptrs)
        return lib.ishara_optimizer_step_groups(h, F(4e-3), F(0.0), grad, st, skip, a["seg_off"], a["groups"], S, a["ws"], N)

    _refused(lib, call(h=N), name, "null handle")
    for off in (4, 8, 12):
        _refused(lib, call(grad=P(BUFS["grad"] + off)), name, "misaligned grad", "16-byte")
    _refused(lib, call(st=P(ST + 2)), name, "misaligned st", "4-byte")
    _refused(lib, call(skip=1), name, "skip_nonfinite needs the record", "null st")
    for k in TABLE:
        _refused(lib, call(**{k: N}), name, f"null {k}")
    _refused(lib, call(seg_off=P(TABLE["seg_off"] + 4)), name, "misaligned seg_off", "8-byte")
    _refused(lib, call(ws=P(TABLE["ws"] + 4)), name, "misaligned ws", "8-byte")
    _refused(lib, call(groups=P(TABLE["groups"] + 2)), name, "misaligned groups", "4-byte")
