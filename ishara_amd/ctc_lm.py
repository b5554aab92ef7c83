"""Character n-gram language models for the CTC prefix beam search, as deterministic automata: the host side of
`ishara_ctc_beam_decode_lm` (csrc/ctc_beam.hip, the AUT instantiations).

The beam's LM term is a function of a hypothesis' prefix only, so an LM is an automaton over the classes:

  LMAutomaton(logp [S, C] f32, next [S, C] i32, start).  Row s of logp is the natural-log probability, fully backed off, of every next
  event in state s: column c != blank is "next character c", column blank is "end of phrase" (the convention of the bigram table of
  ctc_beam.py).  next[s, c] is the state after emitting c in s (column blank unused, 0); start is the state of the empty prefix.
  The bigram table is the case S = C, start = blank, next[s, c] = c, logp = table: LMAutomaton.from_bigram.

CharNGramLM.fit estimates an order-N model (1 <= N <= 8) by interpolated Witten-Bell smoothing:

  Events are the C - 1 non-blank classes and EOS (the blank column).  A phrase is padded with one BOS in front (BOS appears only as the
  oldest symbol of a context) and EOS at the end.  For a context h of k symbols (0 <= k <= N - 1) let c(h, e) be the counts, c(h) their
  sum and t(h) the number of distinct e with c(h, e) > 0; h' is h without its oldest symbol.
    kept context (c(h) >= min_count, not pruned by max_states)   P(e|h) = (c(h, e) + t(h) P(e|h')) / (c(h) + t(h))
    any other context                                           P(e|h) = P(e|h')
    empty context                                               P(e|()) = (c(e) + smoothing) / (n + smoothing C),  n = all events
  Every row sums to 1 and every probability is > 0.  The automaton's states are the empty context and every kept context;
  next[h, c] is the longest kept suffix of h + c truncated to N - 1 symbols.  Every suffix of a kept context is kept (a shorter context
  is seen at least as often, and max_states prunes the longest contexts first), so that suffix is found from the state alone and
  logp[state_after(prefix), c] == logprob(prefix, c) exactly.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

BOS = -1                  # in a context tuple; never an event
MAX_ORDER = 8
MAX_STATES = 1 << 22      # the kernel's limit (include/ishara_hip.h)


class LMAutomaton:
    """logp [S, C] float32, next [S, C] int32 with every entry in [0, S), start in [0, S).  See the module docstring."""

    def __init__(self, logp, next, start: int):
        lp = np.ascontiguousarray(logp, dtype=np.float32)
        nx = np.ascontiguousarray(next, dtype=np.int32)
        if lp.ndim != 2 or nx.shape != lp.shape:
            raise ValueError(f"logp and next must both be [S, C], got {lp.shape} and {nx.shape}")
        S = lp.shape[0]
        if not 1 <= S <= MAX_STATES:
            raise ValueError(f"S={S} states outside 1..{MAX_STATES}")
        if not 0 <= int(start) < S:
            raise ValueError(f"start {start} outside 0..{S - 1}")
        if nx.size and (nx.min() < 0 or nx.max() >= S):
            raise ValueError(f"next holds states outside 0..{S - 1}")
        self.logp, self.next, self.start = lp, nx, int(start)

    @property
    def num_states(self) -> int:
        return self.logp.shape[0]

    @property
    def num_classes(self) -> int:
        return self.logp.shape[1]

    @property
    def table_bytes(self) -> int:
        return self.logp.nbytes + self.next.nbytes

    @classmethod
    def from_bigram(cls, table, blank: Optional[int] = None) -> "LMAutomaton":
        """The [C, C] table of ctc_beam.py (CharBigramLM or an array) as an automaton: the state is the last character."""
        t = np.asarray(table, dtype=np.float32)
        if t.ndim != 2 or t.shape[0] != t.shape[1]:
            raise ValueError(f"an LM table is [C, C], got {t.shape}")
        C = t.shape[0]
        b = getattr(table, "blank", C - 1) if blank is None else int(blank)
        nx = np.tile(np.arange(C, dtype=np.int32), (C, 1))
        nx[:, b] = 0
        return cls(t, nx, b)

    def state_after(self, prefix: Sequence[int]) -> int:
        s = self.start
        for c in prefix:
            s = int(self.next[s, int(c)])
        return s


def _indices(p, char_to_num, C: int, b: int) -> List[int]:
    if isinstance(p, str):
        if char_to_num is None:
            raise ValueError("string phrases need char_to_num")
        seq = [char_to_num[ch] for ch in p]
    else:
        seq = [int(v) for v in p]
    if any(v < 0 or v >= C or v == b for v in seq):
        raise ValueError(f"phrase {p!r}: indices must lie in [0, {C}) and differ from the blank {b}")
    return seq


class CharNGramLM:
    """An order-N character model, interpolated Witten-Bell (module docstring).  `kept` maps a context (a tuple of at most N - 1 classes,
    BOS = -1 only in front) to its float64 count vector [C] (column blank = EOS); `unigram` is the empty context's."""

    def __init__(self, order: int, num_classes: int, blank: int, smoothing: float, unigram, kept: Dict[Tuple[int, ...], np.ndarray]):
        if not 1 <= int(order) <= MAX_ORDER:
            raise ValueError(f"order {order} outside 1..{MAX_ORDER}")
        if smoothing <= 0:
            raise ValueError("smoothing must be > 0 (a zero count would give log 0)")
        self.order, self.num_classes, self.blank, self.smoothing = int(order), int(num_classes), int(blank), float(smoothing)
        self.unigram = np.asarray(unigram, dtype=np.float64)
        self.kept = kept
        self._p0 = (self.unigram + self.smoothing) / (self.unigram.sum() + self.smoothing * self.num_classes)
        self._aut: Optional[LMAutomaton] = None

    # ------------------------------------------------------------------------------------------------ estimation
    @classmethod
    def fit(cls, phrases: Sequence[Union[str, Sequence[int]]], order: int, char_to_num: Optional[Dict[str, int]] = None,
            num_classes: int = 60, smoothing: float = 0.1, blank: Optional[int] = None, min_count: int = 1,
            max_states: Optional[int] = None) -> "CharNGramLM":
        C = int(num_classes)
        b = C - 1 if blank is None else int(blank)
        if not 1 <= int(order) <= MAX_ORDER:
            raise ValueError(f"order {order} outside 1..{MAX_ORDER}")
        if smoothing <= 0:
            raise ValueError("smoothing must be > 0 (a zero count would give log 0)")
        if max_states is not None and max_states < 1:
            raise ValueError("max_states must be >= 1 (the empty context is always a state)")
        counts: Dict[Tuple[int, ...], np.ndarray] = {}
        unigram = np.zeros(C, dtype=np.float64)
        for p in phrases:
            padded = [BOS] + _indices(p, char_to_num, C, b) + [b]           # the last symbol is the EOS event
            for pos in range(1, len(padded)):
                e = padded[pos]
                unigram[e] += 1
                for k in range(1, min(order - 1, pos) + 1):
                    h = tuple(padded[pos - k:pos])
                    v = counts.get(h)
                    if v is None:
                        v = counts[h] = np.zeros(C, dtype=np.float64)
                    v[e] += 1
        kept = {h: v for h, v in counts.items() if v.sum() >= min_count}
        if max_states is not None and 1 + len(kept) > max_states:
            # the rarest of the longest contexts go first; ties by the context itself, so the result does not depend on dict order
            drop = sorted(kept, key=lambda h: (-len(h), kept[h].sum(), h))[:1 + len(kept) - max_states]
            for h in drop:
                del kept[h]
        return cls(order, C, b, smoothing, unigram, kept)

    # ------------------------------------------------------------------------------------------------ direct evaluation
    def _context(self, prefix: Sequence[int]) -> Tuple[int, ...]:
        n = self.order - 1
        hist = (BOS,) + tuple(int(c) for c in prefix)
        return hist[len(hist) - n:] if n < len(hist) else hist

    def _p(self, h: Tuple[int, ...], e: int) -> float:
        if not h:
            return float(self._p0[e])
        v = self.kept.get(h)
        if v is None:
            return self._p(h[1:], e)
        t = float(np.count_nonzero(v))
        return (float(v[e]) + t * self._p(h[1:], e)) / (float(v.sum()) + t)

    def logprob(self, prefix: Sequence[int], c: int) -> float:
        """log P(c | prefix) by the recursion over the count dictionaries (no automaton); c = blank is the end of the phrase."""
        return math.log(self._p(self._context(prefix), int(c)))

    def _pvec(self, h: Tuple[int, ...]) -> np.ndarray:
        """P(. | h) [C] float64: the operations of _p, element by element."""
        if not h:
            return self._p0
        v = self.kept.get(h)
        if v is None:
            return self._pvec(h[1:])
        t = float(np.count_nonzero(v))
        return (v + t * self._pvec(h[1:])) / (float(v.sum()) + t)

    # ------------------------------------------------------------------------------------------------ the automaton
    def _states(self) -> List[Tuple[int, ...]]:
        return [()] + sorted(self.kept, key=lambda h: (len(h), h))

    def _longest_kept_suffix(self, h: Tuple[int, ...]) -> Tuple[int, ...]:
        while h and h not in self.kept:
            h = h[1:]
        return h

    def automaton(self) -> LMAutomaton:
        """States: the empty context (state 0), then the kept contexts by (length, symbols).  Built once and kept."""
        if self._aut is not None:
            return self._aut
        C, b, n = self.num_classes, self.blank, self.order - 1
        states = self._states()
        index = {h: s for s, h in enumerate(states)}
        logp = np.empty((len(states), C), dtype=np.float64)
        nxt = np.zeros((len(states), C), dtype=np.int32)
        for s, h in enumerate(states):
            logp[s] = [math.log(v) for v in self._pvec(h)]                  # math.log, as logprob: the two agree to the bit in fp64
            for c in range(C):
                if c != b:
                    g = h + (c,)
                    nxt[s, c] = index[self._longest_kept_suffix(g[len(g) - n:] if n < len(g) else g)] if n else 0
        self._logp64 = logp
        self._aut = LMAutomaton(logp, nxt, index[self._longest_kept_suffix(self._context(()))])
        return self._aut

    def logp_fp64(self) -> np.ndarray:
        """The automaton's logp before the cast to float32."""
        self.automaton()
        return self._logp64

    # ------------------------------------------------------------------------------------------------ file, sampling
    def save(self, path: str) -> str:
        """One .npz of arrays (no pickled objects): the contexts padded with -2 to N - 1 symbols, their counts, the parameters."""
        hs = sorted(self.kept, key=lambda h: (len(h), h))
        ctx = np.full((len(hs), max(self.order - 1, 1)), -2, dtype=np.int32)
        for k, h in enumerate(hs):
            ctx[k, :len(h)] = h
        cnt = np.stack([self.kept[h] for h in hs]) if hs else np.zeros((0, self.num_classes))
        path = path if path.endswith(".npz") else path + ".npz"
        np.savez(path, order=np.int64(self.order), num_classes=np.int64(self.num_classes), blank=np.int64(self.blank),
                 smoothing=np.float64(self.smoothing), unigram=self.unigram, contexts=ctx, counts=cnt.astype(np.float64))
        return path

    @classmethod
    def load(cls, path: str) -> "CharNGramLM":
        with np.load(path, allow_pickle=False) as z:
            kept = {tuple(int(v) for v in row if v != -2): np.array(c, dtype=np.float64) for row, c in zip(z["contexts"], z["counts"])}
            return cls(int(z["order"]), int(z["num_classes"]), int(z["blank"]), float(z["smoothing"]), z["unigram"], kept)

    def sample(self, rng: np.random.Generator, max_len: int) -> List[int]:
        """One phrase drawn from the model (stops at EOS or max_len)."""
        out: List[int] = []
        while len(out) < max_len:
            p = self._pvec(self._longest_kept_suffix(self._context(out)))
            c = int(rng.choice(self.num_classes, p=p / p.sum()))
            if c == self.blank:
                break
            out.append(c)
        return out


# ---------------------------------------------------------------------------------------------------- which entry point an lm= goes to
def as_automaton(lm) -> Optional[LMAutomaton]:
    """The automaton of a CharNGramLM or an LMAutomaton; None for what the table entry points take (None, an array, a CharBigramLM)."""
    if isinstance(lm, CharNGramLM):
        return lm.automaton()
    return lm if isinstance(lm, LMAutomaton) else None


def entry_point(lm, ragged: bool = False) -> str:
    """The C symbol a decode with this lm= (or with its device form, as ctc_beam.launch asks) launches.  An n-gram or an automaton has
    one entry point, with or without frame lengths; None and the table LMs keep theirs."""
    if isinstance(lm, DeviceAutomaton) or as_automaton(lm) is not None:
        return "ishara_ctc_beam_decode_lm"
    return "ishara_ctc_beam_decode_ex" if ragged else "ishara_ctc_beam_decode"


class DeviceAutomaton:
    """An LMAutomaton's tables on the device (built once per decoder; torch's allocations are at least 256-byte aligned)."""

    def __init__(self, aut: LMAutomaton, C: int, device):
        import torch
        if aut.num_classes != C:
            raise ValueError(f"the lm has {aut.num_classes} classes, the logits {C}")
        self.logp = torch.from_numpy(aut.logp).to(device)
        self.next = torch.from_numpy(aut.next).to(device)
        self.S, self.start = aut.num_states, aut.start
