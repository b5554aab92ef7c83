"""GPU: ishara_ctc_beam_decode, _ex and _lm (csrc/ctc_beam.hip) against the fp64 tracer of ctc_beam_parity.py on every clip of every row of
its case table: beam widths that leave waves empty, with one beam, with one and two, with two; frame counts at, around and past the
log-softmax chunk; alphabets of 2 to 64 classes with the blank first, last and in the middle; n-best depths 1 to W; no LM, the bigram
table and an order-3 automaton; ragged batches.  No clip is skipped: every clip's selection margin exceeds the row's tau, derived on the CPU
from an fp32 twin of the recursion (ctc_beam_parity.py), and every device score must lie within tau / 2 of the fp64 score."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_beam_parity as P
from ishara_amd import _lib
from test_model_gpu import _log_observed

pytestmark = pytest.mark.gpu

GUARD = 4096            # bytes of poison behind the workspace and behind every output
POISON = 0xA5


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(nbytes):
    """A poisoned byte buffer of nbytes (rounded up to 16) + GUARD; the tail must still be poison after the call."""
    n = (nbytes + 15) // 16 * 16
    return torch.full((n + GUARD,), POISON, dtype=torch.uint8, device="cuda"), n


def _decode(lib, case, x, lens, lm):
    """Raw ABI call of the row's entry point on x [B, T, C] -> (idx [B, nbest, T], len [B, nbest], score [B, nbest]) numpy."""
    B, T, Cc = x.shape
    W, nbest = case.W, case.nbest
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    ws_bytes = int(lib.ishara_ctc_beam_workspace_bytes(B, T, Cc, W))
    assert ws_bytes >= 4 * B * (1 + T * W)
    bufs = {name: _guarded(n) for name, n in (("ws", ws_bytes), ("idx", 4 * B * nbest * T), ("len", 4 * B * nbest), ("score", 4 * B * nbest))}
    ptr = {k: C.c_void_p(v[0].data_ptr()) for k, v in bufs.items()}
    fl = torch.from_numpy(lens.astype(np.int32)).cuda() if case.ex else None
    a, b = C.c_float(case.alpha), C.c_float(case.beta)
    if case.lm == "aut3":
        aut = lm.automaton()
        logp, nxt = torch.from_numpy(aut.logp).cuda(), torch.from_numpy(aut.next).cuda()
        rc = lib.ishara_ctc_beam_decode_lm(_lib.ptr(xd), B, T, Cc, case.blank, W, nbest, _lib.ptr(logp), _lib.ptr(nxt), aut.num_states, aut.start,
                                           a, b, ptr["ws"], ptr["idx"], ptr["len"], ptr["score"], _lib.ptr(fl), _stream())
    else:
        lm_d = None if lm is None else torch.from_numpy(np.ascontiguousarray(np.asarray(lm, dtype=np.float32))).cuda()
        if case.ex:
            rc = lib.ishara_ctc_beam_decode_ex(_lib.ptr(xd), B, T, Cc, case.blank, W, nbest, _lib.ptr(lm_d), a, b, ptr["ws"], ptr["idx"],
                                               ptr["len"], ptr["score"], _lib.ptr(fl), _stream())
        else:
            rc = lib.ishara_ctc_beam_decode(_lib.ptr(xd), B, T, Cc, case.blank, W, nbest, _lib.ptr(lm_d), a, b, ptr["ws"], ptr["idx"],
                                            ptr["len"], ptr["score"], _stream())
    _lib.check(rc, "ctc beam decode")
    torch.cuda.synchronize()
    for name, (buf, n) in bufs.items():
        assert bool((buf[n:] == POISON).all()), f"{P.case_id(case)}: the guard behind {name} was written"
    raw = {k: v[0][:v[1]].cpu().numpy() for k, v in bufs.items()}
    idx = raw["idx"][:4 * B * nbest * T].view(np.int32).reshape(B, nbest, T)
    ln = raw["len"][:4 * B * nbest].view(np.int32).reshape(B, nbest)
    sc = raw["score"][:4 * B * nbest].view(np.float32).reshape(B, nbest)
    return idx, ln, sc


def _same_bits(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


@pytest.mark.parametrize("case", P.CASES + P.TIE_CASES, ids=P.case_id)
def test_every_clip_of_the_row_equals_the_tracer(lib, case):
    bt = P.build(case)
    out = _decode(lib, case, bt.x, bt.lens, bt.lm)          # the outputs start as poison: every element must be written
    worst, bad = P.compare(bt, *out)
    print(f"{P.case_id(case)}: E_row {bt.E:.3g} tau {bt.tau:.3g} device score error {worst:.3g} = {worst / (bt.tau / 2):.3f} of tau/2")
    _log_observed(dict(test="ctc_beam_edges", case=P.case_id(case), E_row=bt.E, tau_row=bt.tau, score_err=worst, score_err_over_half_tau=worst / (bt.tau / 2),
                       stale_merges=sum(c["stale"] for c in bt.counters), clips=case.B, failures=len(bad)))
    assert not bad, "\n".join(bad)
    assert _same_bits(out, _decode(lib, case, bt.x, bt.lens, bt.lm)), "two launches differ"


SMALL_ALPHABET = [c for c in P.CASES if c.C == 3 and c.W == 32 and not c.ex][0]


def test_a_clip_alone_equals_the_clip_in_its_batch(lib):
    case = SMALL_ALPHABET
    bt = P.build(case)
    idx, ln, sc = _decode(lib, case, bt.x, bt.lens, bt.lm)
    for b in (0, case.B // 2, case.B - 1):
        one = _decode(lib, case, bt.x[b:b + 1], bt.lens[b:b + 1], bt.lm)
        assert _same_bits(one, (idx[b:b + 1], ln[b:b + 1], sc[b:b + 1])), b
