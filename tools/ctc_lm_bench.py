#!/usr/bin/env python3
"""What the n-gram LM costs the CTC prefix beam search (ishara_ctc_beam_decode_lm against ishara_ctc_beam_decode).  Records

  1. the automaton kernel on a bigram automaton against the table kernel on the same table (the two return the same bits), B = 64 / 256,
     T = 384, C = 60, W = 1 / 4 / 16 / 32, on random N(0, 9) logits and, at B = 256, on confident logits (where most beams keep their
     rank from frame to frame and their rows are not fetched again): the price of fetching the LM rows from memory instead of LDS;
  2. order-3 and order-5 Witten-Bell automata at their own state counts (S and the bytes of the two tables are reported);
  3. BatchedTFLiteModel at configs[4] (fp16, tools/bench_infer.MODEL_KW), batch 256, beam 8: a bigram table against an order-3 LM.

Timing: hip events around INNER back-to-back launches (launch overhead included, divided by INNER), device idle before them.  The two
sides of every comparison alternate round by round in the same process; the median over --reps rounds, the 10th / 90th percentile, and
the median and the extremes of the per-round ratios are kept, so that a ratio can be read against its own run-to-run spread.

    python tools/ctc_lm_bench.py --out profiles/r13_ngram_beam.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_infer import MODEL_KW  # noqa: E402

INNER = 5
T, CN = 384, 60


def _stats(v):
    v = sorted(v)
    n = len(v)
    return dict(median=v[n // 2], p10=v[n // 10], p90=v[min(n - 1, (9 * n) // 10)])


def _phrases(seed, n, classes):
    g = np.random.default_rng(seed)
    return [g.integers(0, classes, int(g.integers(3, 30))).tolist() for _ in range(n)]


def _confident(g, B, sharp=8.0, noise=1.5):
    x = noise * g.standard_normal((B, T, CN))
    for b in range(B):
        t = 0
        while t < T - 8:
            n = int(g.integers(1, 5))
            c = CN - 1 if g.random() < 0.4 else int(g.integers(0, CN - 1))
            x[b, t:min(t + n, T - 8), c] += sharp
            t += n
        x[b, T - 8:, CN - 1] += sharp
    return x.astype(np.float32)


class Launcher:
    """One configuration's buffers and its launch."""

    def __init__(self, lib, x, W, lm, alpha=0.5, beta=0.5):
        import torch
        from ishara_amd import _lib
        from ishara_amd.ctc_beam import lm_to_device
        self.lib, self._lib, self.x, self.W, self.alpha, self.beta = lib, _lib, x, W, alpha, beta
        B = x.shape[0]
        self.lm = lm_to_device(lm, CN, "cuda")
        self.ws = torch.empty(int(lib.ishara_ctc_beam_workspace_bytes(B, T, CN, W)), dtype=torch.uint8, device="cuda")
        self.idx = torch.empty((B, 1, T), dtype=torch.int32, device="cuda")
        self.ln = torch.empty((B, 1), dtype=torch.int32, device="cuda")
        self.sc = torch.empty((B, 1), dtype=torch.float32, device="cuda")
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(self):
        from ishara_amd.ctc_beam import launch
        launch(self.lib, self.x, self.x.shape[0], T, CN, self.W, 1, self.lm, self.alpha, self.beta, self.ws, self.idx, self.ln, self.sc, self.st)

    def result(self):
        import torch
        self.run()
        torch.cuda.synchronize()
        return self.idx.cpu().numpy(), self.ln.cpu().numpy(), self.sc.cpu().numpy().view(np.uint32)


def alternate(sides, reps):
    """sides: {name: Launcher}.  Round by round, every side is timed once (events around INNER launches) -> ms per launch per side."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for s in sides.values():
        s.run()
    ts = {k: [] for k in sides}
    for _ in range(reps):
        for k, s in sides.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(INNER):
                s.run()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / INNER)
    return ts


def _ratio(num, den):
    r = [a / b for a, b in zip(num, den)]
    s = sorted(r)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def bench(args):
    import torch
    from ishara_amd import _lib, get_model
    from ishara_amd.build import source_hash
    from ishara_amd.ctc_beam import CharBigramLM
    from ishara_amd.ctc_lm import CharNGramLM, LMAutomaton
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    from tools.tflite_batch_bench import MAX_FRAMES, make_clips

    lib = _lib.load()
    g = np.random.default_rng(0)
    table = CharBigramLM.fit(_phrases(0, 500, CN - 1), num_classes=CN)
    bigram_aut = LMAutomaton.from_bigram(table)
    out = dict(workload=f"ishara_ctc_beam_decode_lm against ishara_ctc_beam_decode, T={T}, C={CN}, nbest=1, alpha=beta=0.5",
               source_hash=source_hash(),
               timing=f"hip events around {INNER} back-to-back launches / {INNER} (launch overhead included), device idle before them; sides "
                      f"alternate round by round, {args.reps} rounds; ms per launch: median, p10, p90; ratio: median and extremes of the per-round ratios")

    # ---- 1. bigram automaton against the table
    one = {}
    logits = {}
    for B in (64, 256):
        logits[("random", B)] = torch.from_numpy((3.0 * g.standard_normal((B, T, CN))).astype(np.float32)).cuda()
    logits[("confident", 256)] = torch.from_numpy(_confident(g, 256)).cuda()
    for (kind, B), x in logits.items():
        for W in (1, 4, 16, 32):
            sides = dict(table=Launcher(lib, x, W, table), automaton=Launcher(lib, x, W, bigram_aut))
            a, b = sides["table"].result(), sides["automaton"].result()
            same = all(np.array_equal(p, q) for p, q in zip(a, b))
            ts = alternate(sides, args.reps)
            r = _ratio(ts["automaton"], ts["table"])
            d_us = (_stats(ts["automaton"])["median"] - _stats(ts["table"])["median"]) * 1e3 / T
            one[f"{kind}_B{B}_W{W}"] = dict(table_ms=_stats(ts["table"]), automaton_ms=_stats(ts["automaton"]), automaton_over_table=r,
                                            table_us_per_frame=_stats(ts["table"])["median"] * 1e3 / T, extra_us_per_frame=d_us, same_bits=bool(same))
            print(f"{kind} B{B} W{W}: table {_stats(ts['table'])['median']:.3f} ms, automaton {_stats(ts['automaton'])['median']:.3f} ms, "
                  f"ratio {r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}], +{d_us:.3f} us/frame, same bits {same}", flush=True)
    out["bigram_automaton_vs_table"] = one

    # ---- 2. order 3 and order 5 at their own state counts (phrases over 30 classes, so that long contexts repeat)
    two = {}
    ngrams = {o: CharNGramLM.fit(_phrases(1, 3000, 30), order=o, num_classes=CN) for o in (3, 5)}
    for B in (64, 256):
        x = logits[("random", B)]
        for W in (1, 4, 16, 32):
            sides = dict(table=Launcher(lib, x, W, table))
            for o, lm in ngrams.items():
                sides[f"order{o}"] = Launcher(lib, x, W, lm)
            ts = alternate(sides, args.reps)
            rec = dict(table_ms=_stats(ts["table"]))
            for o, lm in ngrams.items():
                aut = lm.automaton()
                rec[f"order{o}"] = dict(S=aut.num_states, table_bytes=aut.table_bytes, ms=_stats(ts[f"order{o}"]),
                                        over_bigram_table=_ratio(ts[f"order{o}"], ts["table"]))
            two[f"random_B{B}_W{W}"] = rec
            print(f"B{B} W{W}: " + ", ".join(f"order {o} S={rec[f'order{o}']['S']} {rec[f'order{o}']['ms']['median']:.3f} ms "
                                                f"(x{rec[f'order{o}']['over_bigram_table']['median']:.4f} of the table)" for o in ngrams), flush=True)
    out["ngram_automata"] = two

    # ---- 3. configs[4] batched inference, beam 8: bigram table against order 3
    _, _, clips, _ = make_clips()
    model = get_model(**MODEL_KW, dtype="f16", max_batch=256, seed=0)
    runners = {}
    for name, lm in (("table", table), ("order3", ngrams[3])):
        r = BatchedTFLiteModel(model, batch_size=256, max_frames=MAX_FRAMES, use_graph=True, beam_width=8, lm=lm, lm_alpha=0.5, lm_beta=0.5)
        r.predict_indices(clips[:512])
        runners[name] = r
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {k: [] for k in runners}
    for _ in range(args.reps):
        for k, r in runners.items():
            torch.cuda.synchronize()
            e0.record(); r._run(0, False); e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    out["batched_tflite_b256_beam8"] = dict(table_replay_ms=_stats(ts["table"]), order3_replay_ms=_stats(ts["order3"]),
                                            order3_over_table=_ratio(ts["order3"], ts["table"]), order3_S=ngrams[3].automaton().num_states,
                                            timing="hip events around one graph replay of slot 0, inputs resident, alternating")
    print(out["batched_tflite_b256_beam8"], flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = bench(a)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
