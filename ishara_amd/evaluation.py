"""Evaluation side of the hot path: the normalised-Levenshtein score of the
inference notebook cell (conv-hybrid-model.ipynb c18:1-15) and the per-epoch transcription report
(CallbackEval, c9:1-29).  Host-side string work; the logits -> index decode it consumes is the HIP
greedy decoder (`Model.decode_batch`).

`edit_alignment` / `ErrorReport` say which characters are confused, dropped or hallucinated: the canonical minimal edit script of a
(prediction, target) pair and its sums over a test set.  They are the host yardstick of ishara_edit_alignment (csrc/score_align.hip)."""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

PAD_TOKEN = "^"        # c1:4
PAD_TOKEN_IDX = 59     # c1:5


def levenshtein(a: Sequence, b: Sequence) -> int:
    """Edit distance with unit insert / delete / substitute costs — `Levenshtein.distance` (c18:1, 9)."""
    if len(a) < len(b):
        a, b = b, a
    if len(b) == 0:
        return len(a)
    prev = np.arange(len(b) + 1)
    bb = np.asarray(list(b), dtype=object)
    for i, ca in enumerate(a, 1):
        cur = np.empty_like(prev)
        cur[0] = i
        sub = prev[:-1] + (bb != ca)
        dele = prev[1:] + 1
        best = np.minimum(sub, dele)
        # insertions are a running minimum along the row
        run = i
        for j in range(1, len(b) + 1):
            run = min(run + 1, best[j - 1])
            cur[j] = run
        prev = cur
    return int(prev[-1])


def normalized_score(prediction: str, target: str) -> float:
    """(len(target) - distance(prediction, target)) / len(target) — c18:9."""
    return (len(target) - levenshtein(prediction, target)) / len(target)


def mean_score(predictions: Iterable[str], targets: Iterable[str]) -> float:
    """np.sum(scores) / len(scores) — c18:13-15."""
    scores = [normalized_score(p, t) for p, t in zip(predictions, targets)]
    return float(np.sum(scores) / len(scores)) if scores else 0.0


N_SYM = 60             # confusion matrix side: the 59 characters and "nothing" at PAD_TOKEN_IDX


class EditAlignment(NamedTuple):
    """The canonical edit script of one (prediction, target) pair.  ops = (matches, substitutions, deletions, insertions); aligned [nb]: the
    predicted symbol at each target position, -1 where the target symbol was deleted; inserted [nb + 1]: extra predicted symbols in front
    of target position j (slot nb: trailing); pairs: the script in target order as (target symbol or 59, predicted symbol or 59)."""
    ops: Tuple[int, int, int, int]
    aligned: np.ndarray
    inserted: np.ndarray
    pairs: List[Tuple[int, int]]


def _strip_pad(target) -> List[int]:
    t = [int(x) for x in target]
    return t[:t.index(PAD_TOKEN_IDX)] if PAD_TOKEN_IDX in t else t


def edit_alignment(pred: Sequence[int], target: Sequence[int]) -> EditAlignment:
    """The full unit-cost Levenshtein table D of prediction a and target b (b ends at its first 59), then the walk from (na, nb) to (0, 0)
    that takes at each cell the first move that applies: diagonal (match / substitution), up (insertion: the prediction holds a symbol
    the target lacks), left (deletion).  Plain and slow on purpose: this is what the device kernel is compared with."""
    a, b = [int(x) for x in pred], _strip_pad(target)
    na, nb = len(a), len(b)
    D = np.zeros((na + 1, nb + 1), dtype=np.int64)
    D[:, 0] = np.arange(na + 1)
    D[0, :] = np.arange(nb + 1)
    for i in range(1, na + 1):
        for j in range(1, nb + 1):
            D[i, j] = min(D[i - 1, j - 1] + (a[i - 1] != b[j - 1]), D[i - 1, j] + 1, D[i, j - 1] + 1)
    aligned = np.full(nb, -1, dtype=np.int64)
    inserted = np.zeros(nb + 1, dtype=np.int64)
    m = s = d = ins = 0
    pairs: List[Tuple[int, int]] = []
    i, j = na, nb
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (a[i - 1] != b[j - 1]):
            aligned[j - 1] = a[i - 1]
            if a[i - 1] == b[j - 1]:
                m += 1
            else:
                s += 1
            pairs.append((b[j - 1], a[i - 1]))
            i, j = i - 1, j - 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            inserted[j] += 1
            ins += 1
            pairs.append((PAD_TOKEN_IDX, a[i - 1]))
            i -= 1
        else:
            aligned[j - 1] = -1
            d += 1
            pairs.append((b[j - 1], PAD_TOKEN_IDX))
            j -= 1
    pairs.reverse()
    return EditAlignment((m, s, d, ins), aligned, inserted, pairs)


def _sym_index(x: int) -> int:
    """A symbol as a confusion-matrix index: anything outside 0..58 counts as "nothing"."""
    return x if 0 <= x < PAD_TOKEN_IDX else PAD_TOKEN_IDX


def _grown(v: np.ndarray, n: int) -> np.ndarray:
    out = np.zeros(n, dtype=np.int64)
    out[:v.shape[0]] = v
    return out


class ErrorReport:
    """Edit operations summed over clips.  confusion [60, 60] int64: row = target symbol, column = predicted symbol, index 59 = nothing
    (row 59: insertions, column 59: deletions).  position_errors [L]: clips whose target position j was substituted or deleted, out of
    position_counts [L] clips that have a position j; insert_positions [L + 1]: inserted symbols by slot."""

    def __init__(self, n_clips: int = 0, matches: int = 0, substitutions: int = 0, deletions: int = 0, insertions: int = 0,
                 confusion=None, position_errors=None, position_counts=None, insert_positions=None):
        self.n_clips, self.matches, self.substitutions = int(n_clips), int(matches), int(substitutions)
        self.deletions, self.insertions = int(deletions), int(insertions)
        self.confusion = np.zeros((N_SYM, N_SYM), np.int64) if confusion is None else np.asarray(confusion, dtype=np.int64).copy()
        if self.confusion.shape != (N_SYM, N_SYM):
            raise ValueError(f"confusion must be [{N_SYM}, {N_SYM}], got {self.confusion.shape}")
        self.position_errors = np.zeros(0, np.int64) if position_errors is None else np.asarray(position_errors, dtype=np.int64).copy()
        self.position_counts = np.zeros(0, np.int64) if position_counts is None else np.asarray(position_counts, dtype=np.int64).copy()
        self.insert_positions = np.zeros(1, np.int64) if insert_positions is None else np.asarray(insert_positions, dtype=np.int64).copy()
        L = self.position_errors.shape[0]
        if self.position_counts.shape != (L,) or self.insert_positions.shape != (L + 1,):
            raise ValueError("position_errors / position_counts must be [L] and insert_positions [L + 1]")

    @classmethod
    def from_alignments(cls, alignments: Sequence[EditAlignment], max_len: Optional[int] = None) -> "ErrorReport":
        L = max([a.aligned.shape[0] for a in alignments] + [max_len or 0])
        r = cls(position_errors=np.zeros(L), position_counts=np.zeros(L), insert_positions=np.zeros(L + 1))
        for al in alignments:
            r.n_clips += 1
            r.matches, r.substitutions = r.matches + al.ops[0], r.substitutions + al.ops[1]
            r.deletions, r.insertions = r.deletions + al.ops[2], r.insertions + al.ops[3]
            j = 0
            for t, p in al.pairs:
                if t == PAD_TOKEN_IDX:                                  # an insertion: no target position
                    r.confusion[PAD_TOKEN_IDX, _sym_index(p)] += 1
                    continue
                deleted = int(al.aligned[j]) == -1
                r.confusion[_sym_index(t), PAD_TOKEN_IDX if deleted else _sym_index(p)] += 1
                r.position_counts[j] += 1
                r.position_errors[j] += int(deleted or p != t)
                j += 1
            r.insert_positions[:al.inserted.shape[0]] += al.inserted
        return r

    @classmethod
    def from_arrays(cls, ops, aligned, inserted, confusion, targets) -> "ErrorReport":
        """From the outputs of ishara_edit_alignment: ops [n, 4], aligned [n, L] (-2 past the target), inserted [n, L + 1], the summed
        matrix, and the pad-59 targets [n, L] the clips were aligned to."""
        ops, aligned, inserted, targets = (np.asarray(v, dtype=np.int64) for v in (ops, aligned, inserted, targets))
        tot = ops.reshape(-1, 4).sum(axis=0)
        has = aligned != -2
        return cls(ops.shape[0], tot[0], tot[1], tot[2], tot[3], confusion,
                   (has & (aligned != targets)).sum(axis=0), has.sum(axis=0), inserted.sum(axis=0))

    def __add__(self, other: "ErrorReport") -> "ErrorReport":
        L = max(self.position_errors.shape[0], other.position_errors.shape[0])
        return ErrorReport(self.n_clips + other.n_clips, self.matches + other.matches, self.substitutions + other.substitutions,
                           self.deletions + other.deletions, self.insertions + other.insertions, self.confusion + other.confusion,
                           _grown(self.position_errors, L) + _grown(other.position_errors, L),
                           _grown(self.position_counts, L) + _grown(other.position_counts, L),
                           _grown(self.insert_positions, L + 1) + _grown(other.insert_positions, L + 1))

    def __eq__(self, other) -> bool:
        if not isinstance(other, ErrorReport):
            return NotImplemented
        L = max(self.position_errors.shape[0], other.position_errors.shape[0])
        return ((self.n_clips, self.matches, self.substitutions, self.deletions, self.insertions)
                == (other.n_clips, other.matches, other.substitutions, other.deletions, other.insertions)
                and np.array_equal(self.confusion, other.confusion)
                and all(np.array_equal(_grown(getattr(self, k), L + e), _grown(getattr(other, k), L + e))
                        for k, e in (("position_errors", 0), ("position_counts", 0), ("insert_positions", 1))))

    __hash__ = None

    def __repr__(self) -> str:
        return (f"ErrorReport(n_clips={self.n_clips}, matches={self.matches}, substitutions={self.substitutions}, "
                f"deletions={self.deletions}, insertions={self.insertions})")

    def per_char(self) -> Dict[str, Dict[int, object]]:
        """{'target': {symbol: {occurrences, correct, substituted, deleted}}, 'inserted': {predicted symbol: count}}, symbols that occur only."""
        c = self.confusion
        tgt = {}
        for t in range(PAD_TOKEN_IDX):
            occ = int(c[t].sum())
            if occ:
                tgt[t] = dict(occurrences=occ, correct=int(c[t, t]), substituted=occ - int(c[t, t]) - int(c[t, PAD_TOKEN_IDX]),
                              deleted=int(c[t, PAD_TOKEN_IDX]))
        return dict(target=tgt, inserted={p: int(n) for p, n in enumerate(c[PAD_TOKEN_IDX]) if n})

    def most_confused(self, k: int = 10) -> List[Tuple[int, int, int]]:
        """The k largest substitution entries (target, predicted, count): off the diagonal, "nothing" excluded; ties by (target, predicted)."""
        c = self.confusion[:PAD_TOKEN_IDX, :PAD_TOKEN_IDX]
        found = [(int(t), int(p), int(c[t, p])) for t, p in zip(*np.nonzero(c)) if t != p]
        return sorted(found, key=lambda e: (-e[2], e[0], e[1]))[:k]

    def format(self, num_to_char: Dict[int, str], k: int = 10) -> str:
        """A small text table: the totals, the k most confused (target, predicted) pairs, the k most deleted and most inserted characters."""
        ch = lambda x: num_to_char.get(int(x), "?")
        lines = [f"clips {self.n_clips}  matches {self.matches}  substitutions {self.substitutions}  deletions {self.deletions}  "
                 f"insertions {self.insertions}",
                 f"{'#':>3} {'tgt':>3} {'pred':>4} {'count':>6}"]
        for n, (t, p, cnt) in enumerate(self.most_confused(k)):
            lines.append(f"{n:>3} {ch(t):>3} {ch(p):>4} {cnt:>6}")
        pc = self.per_char()
        dele = sorted(((v["deleted"], t) for t, v in pc["target"].items() if v["deleted"]), key=lambda e: (-e[0], e[1]))[:k]
        inse = sorted(((n, p) for p, n in pc["inserted"].items()), key=lambda e: (-e[0], e[1]))[:k]
        lines.append("deleted : " + (" ".join(f"{ch(t)}:{n}" for n, t in dele) if dele else "-"))
        lines.append("inserted: " + (" ".join(f"{ch(p)}:{n}" for n, p in inse) if inse else "-"))
        return "\n".join(lines)


def error_report(predictions: Iterable[Sequence[int]], targets: Iterable[Sequence[int]], fallback: bool = False,
                 max_len: Optional[int] = None) -> ErrorReport:
    """The host loop: one ErrorReport from index sequences (targets may be pad-59 rows).  fallback: a prediction shorter than 3 symbols is
    replaced by the TFLite wrapper's constant phrase first (c13:22-23).  max_len: the length of the position arrays (default: the longest target)."""
    phrase = None
    if fallback:
        from .tflite_model import FALLBACK_PHRASE
        phrase = [int(x) for x in FALLBACK_PHRASE]
    als = []
    for p, t in zip(predictions, targets):
        p = [int(x) for x in p]
        als.append(edit_alignment(phrase if (fallback and len(p) < 3) else p, t))
    return ErrorReport.from_alignments(als, max_len)


def make_num_to_char(char_to_num: Dict[str, int]) -> Dict[int, str]:
    """num_to_char with the pad token added at 59 — c1:3-9."""
    m = dict(char_to_num)
    m[PAD_TOKEN] = PAD_TOKEN_IDX
    return {j: i for i, j in m.items()}


def num_to_char_fn(y, num_to_char: Dict[int, str]) -> List[str]:
    """[num_to_char.get(x, "") for x in y] — c8:1-2."""
    return [num_to_char.get(int(x), "") for x in y]


def alignment_table(alignment, num_to_char: Dict[int, str]) -> str:
    """A forced alignment (ishara_amd.ctc_align.Alignment) as a small text table: a header, one line per symbol of the label (its character,
    first and last frame, frame count, confidence) and the log-probability of the path; a label without an alignment says so."""
    lines = [f"{'#':>3} {'sym':>3} {'first':>5} {'last':>5} {'frames':>6} {'conf':>6}"]
    for i, (sym, start, end, conf) in enumerate(alignment.spans):
        lines.append(f"{i:>3} {num_to_char.get(int(sym), '?'):>3} {start:>5} {end - 1:>5} {end - start:>6} {conf:>6.3f}")
    lines.append("no alignment" if alignment.score <= -1e29 else f"log p(path) = {alignment.score:.3f}")
    return "\n".join(lines)


class CallbackEval:
    """Displays a batch of outputs after every epoch (c9:1-29): saves the weights, decodes every batch of
    `dataset` greedily and prints target / prediction pairs.  `model` is an `ishara_amd.Model`."""

    def __init__(self, dataset: Iterable, num_to_char: Dict[int, str], n_show: int = 32,
                 weights_path: Optional[str] = "model.npz", printer: Callable[[str], None] = print,
                 error_report: bool = False, n_confusions: int = 10, averaged: bool = False):
        """averaged: run the epoch's evaluation on the moving average of the weights (Optimizer(use_ema=True)): the weights file, the
        forward passes, the decodes and the report all happen inside `model.averaged_weights()`, which puts the training weights back
        afterwards.  error_report: also align every decode with its label on the device (ishara_amd.score.edit_alignment_device, no fallback), print
        the merged ErrorReport's table (n_confusions pairs) after the transcript, keep it as `last_report` and log the operation totals."""
        self.dataset = dataset
        self.num_to_char = num_to_char
        self.n_show = n_show
        self.weights_path = weights_path
        self.printer = printer
        self.model = None
        self.last_score: Optional[float] = None
        self.error_report = error_report
        self.n_confusions = n_confusions
        self.last_report: Optional[ErrorReport] = None
        self.averaged = averaged

    def _align_batch(self, model, logits, y, confusion):
        """One validation batch decoded once on the device and aligned with its labels there: the decodes as decode_batch returns them, and
        (ops, aligned, inserted, pad-59 labels) on the host; the matrix stays on the device."""
        import torch
        from .score import edit_alignment_device
        idx, ln = model._decode_device(logits)
        tg = torch.as_tensor(np.asarray(y.cpu() if hasattr(y, "cpu") else y)).to(device=idx.device, dtype=torch.int32).contiguous()
        ops, aligned, inserted, _ = edit_alignment_device(idx, ln, tg, fallback=False, confusion=confusion)
        idx, ln = idx.cpu().numpy(), ln.cpu().numpy()
        decodes = [idx[b, :ln[b]].astype(np.int64) for b in range(idx.shape[0])]
        return decodes, (ops.cpu().numpy(), aligned.cpu().numpy(), inserted.cpu().numpy(), tg.cpu().numpy())

    def set_model(self, model):
        self.model = model

    def on_epoch_begin(self, epoch: int, logs=None):
        pass

    def on_epoch_end(self, epoch: int, logs=None):
        if not self.averaged:
            return self._evaluate_epoch(epoch, logs)
        with self.model.averaged_weights():
            return self._evaluate_epoch(epoch, logs)

    def _evaluate_epoch(self, epoch: int, logs=None):
        model = self.model
        if self.weights_path:
            model.save_weights(self.weights_path)                                   # c9:10
        predictions, targets = [], []
        parts, confusion = [], None
        for batch in self.dataset:                                                  # c9:13-21; (X, y) or (X, y, frame_lengths)
            X, y = batch[0], batch[1]
            logits = model(X, training=False, **({"frame_lengths": batch[2]} if len(batch) == 3 else {}))
            if self.error_report:
                if confusion is None:
                    import torch
                    confusion = torch.zeros((N_SYM, N_SYM), dtype=torch.int32, device=model.device)
                decodes, part = self._align_batch(model, logits, y, confusion)
                parts.append(part)
            else:
                decodes = model.decode_batch(logits)
            for idx in decodes:
                predictions.append("".join(num_to_char_fn(idx, self.num_to_char)))
            for label in np.asarray(y.cpu() if hasattr(y, "cpu") else y):
                targets.append("".join(num_to_char_fn(label, self.num_to_char)))    # includes the pad characters, as c9:20 does
        self.printer("-" * 100)
        for i in range(min(self.n_show, len(predictions))):                         # c9:24-27
            self.printer(f"Target    : {targets[i]}")
            self.printer(f"Prediction: {predictions[i]}, len: {len(predictions[i])}")
            self.printer("-" * 100)
        stripped = [t.replace(PAD_TOKEN, "") for t in targets]
        pairs = [(p, t) for p, t in zip(predictions, stripped) if len(t) > 0]
        self.last_score = mean_score([p for p, _ in pairs], [t for _, t in pairs])
        if logs is not None:
            logs["val_levenshtein"] = self.last_score
        if self.error_report:
            rep = ErrorReport()
            if parts:
                ops, aligned, inserted, tg = (np.concatenate([p[k] for p in parts]) for k in range(4))
                rep = ErrorReport.from_arrays(ops, aligned, inserted, confusion.cpu().numpy(), tg)
            self.last_report = rep
            self.printer(rep.format(self.num_to_char, self.n_confusions))
            if logs is not None:
                logs["val_substitutions"], logs["val_deletions"], logs["val_insertions"] = rep.substitutions, rep.deletions, rep.insertions


class TrainStateCheckpoint:
    """Keras-style callback: `model.save_state(path)` at the end of every `every_epochs`-th epoch, so that a preempted run resumes with
    `load_state(path)` and `fit(..., initial_epoch=...)`.  `path` may hold `{epoch}` (1-based, as Keras' ModelCheckpoint formats it).  The
    epoch must end on a whole accumulation cycle (save_state refuses in the middle of one)."""

    def __init__(self, path: str, every_epochs: int = 1):
        if every_epochs < 1:
            raise ValueError("every_epochs must be >= 1")
        self.path, self.every_epochs = path, int(every_epochs)
        self.model = None
        self.last_path: Optional[str] = None

    def set_model(self, model): self.model = model
    def on_train_begin(self, logs=None): pass
    def on_train_end(self, logs=None): pass
    def on_epoch_begin(self, epoch, logs=None): pass
    def on_train_batch_end(self, batch, logs=None): pass

    def on_epoch_end(self, epoch, logs=None):
        if (epoch + 1) % self.every_epochs == 0:
            self.last_path = self.model.save_state(self.path.format(epoch=epoch + 1))
