"""Training-loop state around the flat fp32 gradient: host references of the device kernels in csrc/grad_ops.hip and of the clipped /
skipped optimizer step (numpy, in the manner of ctc_beam.prefix_beam_search and ctc_align.viterbi_align), and the resumable-state file
of `Model.save_state` / `load_state` (pack / unpack / validate on numpy arrays: nothing here needs a GPU).

Semantics (include/ishara_hip.h):
  norm      = grad_scale * sqrt(sum_i g[i]^2), every square and the sum in fp64, stored as fp32
  coef      = grad_scale * min(1, clip_norm / (norm + 1e-6)) when clip_norm > 0 (torch.nn.utils.clip_grad_norm_), else grad_scale
  nonfinite = number of NaN / +-Inf elements (saturating at INT32_MAX)
  the step  = Lookahead(RectifiedAdam) on g * coef; with skip_nonfinite and nonfinite > 0 it writes nothing, counts itself in `skipped`
              and still consumes its iteration number (the counter lives on the host, which does not read the device record).
"""
from __future__ import annotations

import fnmatch
import json
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

FORMAT_VERSION = 1
GRAD_WG_SPAN = 1024       # elements one workgroup covers per grid-stride round (csrc/grad_ops.hip)
GRAD_GRID_CAP = 2048      # most workgroups of a launch (csrc/grad_ops.hip)
INT32_MAX = 2 ** 31 - 1

ARRAYS = ("params", "opt_m", "opt_v", "opt_slow")
SCALARS = ("format_version", "iterations", "steps", "step_seed", "learning_rate", "weight_decay", "apply_weight_decay",
           "global_clipnorm", "skip_nonfinite", "accumulate_steps", "skipped")
ENTRY_KEYS = ("entry_names", "entry_shapes", "entry_offsets", "entry_trainable")


def grad_stats_workspace_bytes(n: int) -> int:
    """what ishara_grad_stats_workspace_bytes(n) returns: one 16-byte row per workgroup of the launch"""
    return 16 * min(GRAD_GRID_CAP, -(-int(n) // GRAD_WG_SPAN))


def grad_stats_reference(g: Union[np.ndarray, Sequence[np.ndarray]], grad_scale: float = 1.0, clip_norm: float = 0.0) -> Dict[str, float]:
    """{norm, coef, nonfinite} of the gradient `g` (one array, or a list of arrays taken as one vector) as ishara_gradient_stats defines them.
    The sum of squares is taken in fp64; norm and coef are rounded as the kernel rounds them (fp32 store, fp32 coef arithmetic)."""
    parts = [g] if isinstance(g, np.ndarray) else list(g)
    ss, bad = 0.0, 0
    for p in parts:
        p = np.asarray(p, dtype=np.float32).reshape(-1)
        d = p.astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            ss += float(np.sum(d * d))
        bad += int(np.count_nonzero(~np.isfinite(p)))
    gs = np.float32(grad_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        norm = np.float32(float(gs) * math.sqrt(ss)) if not math.isnan(ss) else np.float32(np.nan)
        coef = gs
        if clip_norm > 0:
            coef = gs * min(np.float32(1.0), np.float32(clip_norm) / (norm + np.float32(1e-6)))
    return dict(norm=float(norm), coef=float(np.float32(coef)), nonfinite=min(bad, INT32_MAX))


def radam_coeffs(step: int, beta1: float = 0.9, beta2: float = 0.999, sma_threshold: float = 4.0) -> dict:
    """the host-side scalars of step `step` (1-based): bias corrections, rectification term and whether it applies"""
    b1p, b2p = beta1 ** step, beta2 ** step
    sma_inf = 2.0 / (1.0 - beta2) - 1.0
    sma_t = sma_inf - 2.0 * step * b2p / (1.0 - b2p)
    rect = sma_t >= sma_threshold
    r_t = math.sqrt(max((sma_t - 4.0) / (sma_inf - 4.0) * (sma_t - 2.0) / (sma_inf - 2.0) * sma_inf / sma_t, 0.0)) if rect else 0.0
    return dict(c1=1.0 / (1.0 - b1p), c2=1.0 / (1.0 - b2p), r_t=r_t, rect=bool(rect))


def step_state_init(theta: np.ndarray) -> dict:
    """{m, v, slow, step, skipped} before the first step: zero moments, the Lookahead slow weights at theta_0"""
    return dict(m=np.zeros_like(theta), v=np.zeros_like(theta), slow=theta.copy(), step=0, skipped=0)


def clipped_step_reference(theta: np.ndarray, grad: np.ndarray, state: dict, lr: float, coef: float = 1.0, nonfinite: int = 0,
                           skip_nonfinite: bool = False, weight_decay: float = 0.0, beta1: float = 0.9, beta2: float = 0.999,
                           eps: float = 1e-7, sync_period: int = 5, slow_step: float = 0.5) -> np.ndarray:
    """One ishara_optimizer_step_ex in numpy fp32: Lookahead(RectifiedAdam(sma_threshold=4), sync_period=5) on grad * coef -> the new theta;
    `state` (step_state_init) is updated in place.  With skip_nonfinite and nonfinite > 0: theta and the slots stay, state["skipped"] and
    state["step"] advance."""
    state["step"] += 1
    if skip_nonfinite and nonfinite > 0:
        state["skipped"] += 1
        return theta
    c = radam_coeffs(state["step"], beta1, beta2)
    g = grad * np.float32(coef)
    state["m"] = beta1 * state["m"] + (1 - beta1) * g
    state["v"] = beta2 * state["v"] + (1 - beta2) * g * g
    m_hat = state["m"] * np.float32(c["c1"])
    if c["rect"]:
        upd = np.float32(c["r_t"]) * m_hat / (np.sqrt(state["v"] * np.float32(c["c2"])) + np.float32(eps))
    else:
        upd = m_hat
    if weight_decay:
        upd = upd + np.float32(weight_decay) * theta
    theta = theta - np.float32(lr) * upd
    if state["step"] % sync_period == 0:
        state["slow"] = state["slow"] + np.float32(slow_step) * (theta - state["slow"])
        theta = state["slow"].copy()
    return theta


# ---------------------------------------------------------------------------------- the moving average of the weights (csrc/weight_avg.hip)
def ema_alpha(n: int, momentum: float, warmup: bool = False) -> np.float32:
    """The smoothing factor of update number n + 1 (n updates applied so far): alpha = (float)(1 - d), d = (double)(float)momentum, under
    warm-up min(d, (1 + n) / (10 + n)) (tf.train.ExponentialMovingAverage's num_updates rule); evaluated in fp64 like the kernel."""
    d = float(np.float32(momentum))
    if warmup:
        d = min(d, (1.0 + float(n)) / (10.0 + float(n)))
    return np.float32(1.0 - d)


def ema_state_init() -> dict:
    """the zeroed ishara_ema_state record"""
    return dict(updates=0, alpha=np.float32(0.0), overwrote=0)


def ema_reference(avg: np.ndarray, theta: np.ndarray, state: dict, momentum: float, warmup: bool = False, overwrite_every: int = 0,
                  nonfinite: int = 0, skip_nonfinite: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """One ishara_weight_average in numpy fp32 -> (avg, theta); `state` ({updates, alpha, overwrote}, ema_state_init) is updated in
    place.  avg + alpha * (theta - avg): numpy rounds each of the three operations to fp32 and fuses nothing, as the kernel.  With
    skip_nonfinite and nonfinite > 0 the inputs come back as they are, updates and alpha stay, overwrote = 0.  With overwrite_every = N > 0
    and the new update count a multiple of N, theta comes back as a copy of the new average."""
    if skip_nonfinite and nonfinite > 0:
        state["overwrote"] = 0
        return avg, theta
    avg = np.asarray(avg, dtype=np.float32)
    theta = np.asarray(theta, dtype=np.float32)
    alpha = ema_alpha(state["updates"], momentum, warmup)
    with np.errstate(over="ignore", invalid="ignore"):
        avg = avg + alpha * (theta - avg)
    state["updates"] += 1
    state["alpha"] = alpha
    state["overwrote"] = 1 if overwrite_every > 0 and state["updates"] % overwrite_every == 0 else 0
    if state["overwrote"]:
        theta = avg.copy()
    return avg, theta


# ---------------------------------------------------------------------------------- adversarial weight perturbation (csrc/awp.hip)
AWP_CHUNK = 4096          # elements of one chunk of a segment (csrc/awp.hip): a segment longer than this is summed in pieces


def awp_segments(entries: Iterable[Tuple[str, tuple, int, bool]], n_train: int) -> np.ndarray:
    """seg_off of ishara_awp_perturb, int64 [S + 1]: the offsets of the trainable entries in offset order, then n_train.  The trainable
    entries must tile [0, n_train) exactly (they do: the parameter layout puts them in front of the BatchNorm moving statistics)."""
    segs = sorted((int(o), int(np.prod(s))) for _, s, o, t in entries if t)
    pos = 0
    for o, size in segs:
        if o != pos or size < 1:
            raise ValueError(f"awp_segments: the trainable entries do not tile [0, {n_train}): an entry of {size} elements at offset {o}, expected offset {pos}")
        pos += size
    if pos != int(n_train) or not segs:
        raise ValueError(f"awp_segments: the trainable entries cover [0, {pos}), not [0, {n_train})")
    return np.array([o for o, _ in segs] + [pos], dtype=np.int64)


def _awp_sumsq(x: np.ndarray) -> float:
    """sum of (double)x[i]^2, exactly rounded (each square of an fp32 value is exact in fp64); inf / nan when the data holds one"""
    d = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = d * d
    if not np.isfinite(sq).all():
        return float("nan") if np.isnan(sq).any() else float("inf")
    try:
        return math.fsum(sq.tolist())
    except OverflowError:
        return float("inf")


def awp_reference(w: np.ndarray, g: np.ndarray, seg_off: Sequence[int], delta: float, eps: float, relative: bool = False
                  ) -> Tuple[np.ndarray, np.ndarray, dict]:
    """One ishara_awp_perturb in numpy -> (w_adv float32 [n], scale float32 [S], {grad_norm, delta_norm, perturbed, zeroed}).  Per
    segment s = [seg_off[s], seg_off[s + 1]): ss_g = sum g^2 (and ss_w = sum w^2 with `relative`) in fp64 through math.fsum; a sum that is
    not finite zeroes the segment (scale 0, the weights keep their bits); else scale = fp32(delta / (sqrt(ss_g) + eps)), with `relative`
    fp32(delta * sqrt(ss_w) / (sqrt(ss_g) + eps)), delta and eps taken as fp32 values like the kernel's arguments, and
    w_adv = fp32(w + fp32(scale * g)): numpy rounds each operation to fp32 and fuses nothing.  The two norms sum over the segments that
    were not zeroed, in segment order."""
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    seg_off = [int(o) for o in seg_off]
    d64, e64 = float(np.float32(delta)), float(np.float32(eps))
    out = w.copy()
    scale = np.zeros(len(seg_off) - 1, dtype=np.float32)
    tot_g = tot_d = 0.0
    zeroed = 0
    for s, (lo, hi) in enumerate(zip(seg_off[:-1], seg_off[1:])):
        ss_g = _awp_sumsq(g[lo:hi])
        ss_w = _awp_sumsq(w[lo:hi]) if relative else 0.0
        if not math.isfinite(ss_g) or not math.isfinite(ss_w):
            zeroed += 1
            continue
        num = d64 * math.sqrt(ss_w) if relative else d64
        scale[s] = np.float32(num / (math.sqrt(ss_g) + e64))
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            step = scale[s] * g[lo:hi]
            out[lo:hi] = w[lo:hi] + step
        tot_g += ss_g
        tot_d += float(scale[s]) ** 2 * ss_g
    stats = dict(grad_norm=float(np.float32(math.sqrt(tot_g))), delta_norm=float(np.float32(math.sqrt(tot_d))),
                 perturbed=len(scale) - zeroed, zeroed=zeroed)
    return out, scale, stats


# ---------------------------------------------------------------------------------- optimizer parameter groups (csrc/optimizer.hip)
PARAM_GROUP_DTYPE = np.dtype([("lr_scale", "<f4"), ("wd_scale", "<f4"), ("frozen", "<i4"), ("reserved", "<i4")])      # ishara_param_group
PARAM_GROUP_FIELDS = ("match", "lr_scale", "weight_decay_scale", "trainable")


def _scale_f32(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"param_groups: {what} must be a number, got {v!r}")
    with np.errstate(over="ignore", under="ignore"):
        f = float(np.float32(v))
    if not (math.isfinite(f) and f >= 0):
        raise ValueError(f"param_groups: {what} must be finite and >= 0 (as float32), got {v!r}")
    return float(v)


def check_param_groups(groups) -> Optional[List[dict]]:
    """The checked form of Optimizer.param_groups: None, or a list of {"match": [pattern, ...], "lr_scale", "weight_decay_scale",
    "trainable"} with the defaults (1.0, 1.0, True) filled in.  Anything else raises ValueError."""
    if groups is None:
        return None
    if not isinstance(groups, (list, tuple)):
        raise ValueError(f"param_groups must be None or a list of dicts, got {type(groups).__name__}")
    out = []
    for i, g in enumerate(groups):
        if not isinstance(g, dict):
            raise ValueError(f"param_groups[{i}] must be a dict, got {type(g).__name__}")
        unknown = sorted(set(g) - set(PARAM_GROUP_FIELDS))
        if unknown:
            raise ValueError(f"param_groups[{i}]: unknown key(s) {unknown}; the keys are {list(PARAM_GROUP_FIELDS)}")
        if "match" not in g:
            raise ValueError(f"param_groups[{i}] has no 'match'")
        pats = [g["match"]] if isinstance(g["match"], str) else g["match"]
        if not isinstance(pats, (list, tuple)) or not pats or not all(isinstance(p, str) and p for p in pats):
            raise ValueError(f"param_groups[{i}]: 'match' must be a pattern or a non-empty list of patterns, got {g['match']!r}")
        trainable = g.get("trainable", True)
        if not isinstance(trainable, (bool, np.bool_)):
            raise ValueError(f"param_groups[{i}]: 'trainable' must be a bool, got {trainable!r}")
        out.append(dict(match=list(pats), lr_scale=_scale_f32(g.get("lr_scale", 1.0), f"lr_scale of group {i}"),
                        weight_decay_scale=_scale_f32(g.get("weight_decay_scale", 1.0), f"weight_decay_scale of group {i}"), trainable=bool(trainable)))
    return out


def param_groups_json(groups) -> str:
    """the canonical text of checked groups: the state-file entry, and the key the model compares to see a change by value"""
    return json.dumps(check_param_groups(groups), sort_keys=True)


def _trainable_names(entries) -> List[str]:
    return [n for _, n in sorted((int(o), n) for n, _, o, t in entries if t)]


def resolve_param_groups(entries, groups) -> Dict[str, dict]:
    """{trainable entry name, in offset order: {lr_scale, weight_decay_scale, trainable}}: fnmatch.fnmatchcase of every pattern over the
    names of the trainable entries, the first matching group wins, an unmatched entry gets (1.0, 1.0, True).  A pattern that matches no
    trainable entry (a typo, or one that only hits the BatchNorm moving statistics) raises and names the pattern."""
    groups = check_param_groups(groups) or []
    names = _trainable_names(entries)
    for i, g in enumerate(groups):
        for p in g["match"]:
            if not any(fnmatch.fnmatchcase(n, p) for n in names):
                raise ValueError(f"param_groups[{i}]: the pattern {p!r} matches no trainable entry")
    out = {}
    for n in names:
        hit = next((g for g in groups if any(fnmatch.fnmatchcase(n, p) for p in g["match"])), None)
        out[n] = dict(lr_scale=hit["lr_scale"] if hit else 1.0, weight_decay_scale=hit["weight_decay_scale"] if hit else 1.0,
                      trainable=hit["trainable"] if hit else True)
    return out


def param_group_rows(entries, n_train: int, groups) -> Tuple[np.ndarray, np.ndarray]:
    """(seg_off, rows) of ishara_optimizer_step_groups: awp_segments of the entries and one PARAM_GROUP_DTYPE row per segment."""
    seg_off = awp_segments(entries, n_train)
    res = resolve_param_groups(entries, groups)
    rows = np.zeros(len(seg_off) - 1, dtype=PARAM_GROUP_DTYPE)
    for s, r in enumerate(res.values()):
        rows[s] = (np.float32(r["lr_scale"]), np.float32(r["weight_decay_scale"]), 0 if r["trainable"] else 1, 0)
    return seg_off, rows


def no_decay_groups(entries) -> List[dict]:
    """one group with weight_decay_scale = 0 naming every trainable entry of at most one dimension (biases, gamma, beta): the
    weight-decay exclusion of the AdamW recipes, for Optimizer(param_groups=...) with apply_weight_decay"""
    return [dict(match=[n for n, s, _, t in entries if t and len(tuple(s)) <= 1], weight_decay_scale=0.0)]


def param_groups_reference(theta: np.ndarray, grad: np.ndarray, state: dict, seg_off: Sequence[int], rows: np.ndarray, lr: float, coef: float = 1.0,
                           nonfinite: int = 0, skip_nonfinite: bool = False, weight_decay: float = 0.0, **kw) -> np.ndarray:
    """One ishara_optimizer_step_groups in numpy -> the new theta; `state` (step_state_init) is updated in place.  clipped_step_reference
    runs once per distinct unfrozen row on copies, with lr' = fp32(lr) * fp32(lr_scale) and wd' = fp32(wd) * fp32(wd_scale) (one fp32
    product each; wd' = 0 is a step without decay), and the segments are stitched from the run of their row; a frozen segment keeps
    theta and the three slots as they came.  A skipped step advances the step number and `skipped` once."""
    rows = np.asarray(rows, dtype=PARAM_GROUP_DTYPE)
    seg_off = [int(o) for o in seg_off]
    if skip_nonfinite and nonfinite > 0:
        state["step"] += 1
        state["skipped"] += 1
        return theta
    out = {k: np.array(state[k], dtype=np.float32) for k in ("m", "v", "slow")}
    new_theta = np.array(theta, dtype=np.float32)
    runs = {}
    for s, r in enumerate(rows):
        if r["frozen"] != 0:
            continue
        key = (r["lr_scale"].tobytes(), r["wd_scale"].tobytes())
        if key not in runs:
            st = dict(m=state["m"].copy(), v=state["v"].copy(), slow=state["slow"].copy(), step=state["step"], skipped=state["skipped"])
            with np.errstate(over="ignore", invalid="ignore", under="ignore"):
                lr_s, wd_s = np.float32(lr) * r["lr_scale"], np.float32(weight_decay) * r["wd_scale"]
                th = clipped_step_reference(np.array(theta, dtype=np.float32), grad, st, float(lr_s), coef=coef, weight_decay=float(wd_s), **kw)
            runs[key] = (th, st)
        th, st = runs[key]
        lo, hi = seg_off[s], seg_off[s + 1]
        new_theta[lo:hi] = th[lo:hi]
        for k in out:
            out[k][lo:hi] = st[k][lo:hi]
    state.update(out)
    state["step"] += 1
    return new_theta


def mask_reference(g: np.ndarray, seg_off: Sequence[int], rows: np.ndarray) -> np.ndarray:
    """ishara_gradient_mask_groups in numpy: a copy of g with +0.0 over the frozen segments, every other word untouched"""
    out = np.array(g, dtype=np.float32)
    for s, r in enumerate(np.asarray(rows, dtype=PARAM_GROUP_DTYPE)):
        if r["frozen"] != 0:
            out[int(seg_off[s]):int(seg_off[s + 1])] = np.float32(0.0)
    return out


# ---------------------------------------------------------------------------------- the state file
EMA_KEYS = ("ema_avg", "ema_updates", "ema_momentum", "ema_warmup", "ema_overwrite_frequency", "use_ema")
AWP_KEYS = ("awp_delta", "awp_eps", "awp_start_step", "awp_relative")
PARAM_GROUP_KEYS = ("param_groups",)
MWER_KEYS = ("mwer",)          # the seven Optimizer(mwer_*) options as one JSON text (ishara_amd/mwer.py check_options)


KD_KEYS = ("kd",)              # the five Optimizer(kd_*) options as one JSON text (ishara_amd/kd.py check_options); never the teacher


class TrainStateError(ValueError):
    pass


def mwer_json(options: dict) -> str:
    """the canonical text of the seven mwer_* options in a state file"""
    from .mwer import check_options
    return json.dumps(check_options(**options), sort_keys=True)


def mwer_options(text: str) -> dict:
    """the checked options of that text; a key that is not one of the seven is refused (TypeError)"""
    from .mwer import check_options
    d = json.loads(text)
    if not isinstance(d, dict):
        raise ValueError(f"expected a JSON object, got {type(d).__name__}")
    return check_options(**d)


def kd_json(options: dict) -> str:
    """the canonical text of the five kd_* options in a state file"""
    from .kd import check_options
    return json.dumps(check_options(**options), sort_keys=True)


def kd_options(text: str) -> dict:
    """the checked options of that text; a key that is not one of the five is refused (TypeError)"""
    from .kd import check_options
    d = json.loads(text)
    if not isinstance(d, dict):
        raise ValueError(f"expected a JSON object, got {type(d).__name__}")
    return check_options(**d)


def _entry_arrays(entries: Iterable[Tuple[str, tuple, int, bool]]) -> Dict[str, np.ndarray]:
    entries = list(entries)
    shapes = np.full((len(entries), 2), -1, dtype=np.int64)
    for i, (_, s, _, _) in enumerate(entries):
        shapes[i, :len(s)] = s
    return dict(entry_names=np.array([n for n, _, _, _ in entries], dtype=np.str_), entry_shapes=shapes,
                entry_offsets=np.array([o for _, _, o, _ in entries], dtype=np.int64),
                entry_trainable=np.array([bool(t) for _, _, _, t in entries], dtype=np.bool_))


def pack_state(entries, params: np.ndarray, opt_m: np.ndarray, opt_v: np.ndarray, opt_slow: np.ndarray, *, iterations: int, steps: int,
               step_seed: int, learning_rate: float, weight_decay: float, apply_weight_decay: bool = False,
               global_clipnorm: Optional[float] = None, skip_nonfinite: bool = False, accumulate_steps: int = 1, skipped: int = 0,
               ema_avg: Optional[np.ndarray] = None, ema_updates: int = 0, use_ema: bool = True, ema_momentum: float = 0.99,
               ema_warmup: bool = False, ema_overwrite_frequency: Optional[int] = None, awp_delta: Optional[float] = None,
               awp_eps: float = 1e-4, awp_start_step: int = 0, awp_relative: bool = False, param_groups=None, mwer: Optional[dict] = None,
               kd: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """The arrays of one state file (np.savez(path, **pack_state(...))): the flat fp32 `params` (BatchNorm moving statistics included), the
    three optimizer slots, the counters, the hyper-parameters, the format version and the entry list the buffers were laid out by.  With
    `ema_avg` (the moving average of the trainable prefix, when one exists) the file also holds EMA_KEYS: the average, its update count
    and the four settings; without it the key set is what it was before the average existed.  With `awp_delta` (adversarial weight
    perturbation is configured) it holds AWP_KEYS, the four options; AWP has no other state.  With `param_groups` (the optimizer's
    parameter groups are set) it holds PARAM_GROUP_KEYS: the JSON text of the checked list.  With `mwer` (minimum-risk training is
    configured: the dict of the seven mwer_* options) it holds MWER_KEYS: their JSON text; it has no other state.  With `kd` (distillation
    is configured: the dict of the five kd_* options) it holds KD_KEYS: their JSON text; the teacher is not saved."""
    out = {k: np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for k, v in zip(ARRAYS, (params, opt_m, opt_v, opt_slow))}
    out.update(_entry_arrays(entries))
    out.update(format_version=np.int64(FORMAT_VERSION), iterations=np.int64(iterations), steps=np.int64(steps), step_seed=np.int64(step_seed),
               learning_rate=np.float64(learning_rate), weight_decay=np.float64(weight_decay), apply_weight_decay=np.bool_(apply_weight_decay),
               global_clipnorm=np.float64(0.0 if global_clipnorm is None else global_clipnorm), skip_nonfinite=np.bool_(skip_nonfinite),
               accumulate_steps=np.int64(accumulate_steps), skipped=np.int64(skipped))
    if ema_avg is not None:
        a = np.asarray(ema_avg)
        out.update(ema_avg=np.ascontiguousarray(a).reshape(-1) if a.dtype == np.float32 else a, ema_updates=np.int64(ema_updates),
                   use_ema=np.bool_(use_ema), ema_momentum=np.float64(ema_momentum), ema_warmup=np.bool_(ema_warmup),
                   ema_overwrite_frequency=np.int64(0 if ema_overwrite_frequency is None else ema_overwrite_frequency))
    if awp_delta is not None:
        out.update(awp_delta=np.float64(awp_delta), awp_eps=np.float64(awp_eps), awp_start_step=np.int64(awp_start_step), awp_relative=np.bool_(awp_relative))
    if param_groups is not None:
        out.update(param_groups=np.array(param_groups_json(param_groups), dtype=np.str_))
    if mwer is not None:
        out.update(mwer=np.array(mwer_json(mwer), dtype=np.str_))
    if kd is not None:
        out.update(kd=np.array(kd_json(kd), dtype=np.str_))
    validate_state(out, entries)
    return out


def validate_state(z, entries) -> None:
    """Refuses, with a message, a state whose version is unknown, that lacks an array, or whose entry list or buffer sizes are not the
    model's (`entries` = [(name, shape, offset, trainable)]).  `z`: a mapping of name -> array (a dict, or an open .npz)."""
    keys = set(z.files) if hasattr(z, "files") else set(z)
    if "format_version" not in keys:
        raise TrainStateError("train state: missing entry 'format_version' (not a state file of save_state?)")
    ver = int(z["format_version"])
    if ver != FORMAT_VERSION:
        raise TrainStateError(f"train state: unknown format version {ver} (this build reads version {FORMAT_VERSION})")
    for k in ARRAYS + SCALARS + ENTRY_KEYS:
        if k not in keys:
            raise TrainStateError(f"train state: missing entry '{k}'")
    entries = list(entries)
    want = _entry_arrays(entries)
    names, shapes = [str(n) for n in z["entry_names"]], np.asarray(z["entry_shapes"])
    if len(names) != len(entries):
        raise TrainStateError(f"train state: {len(names)} parameter entries, the model has {len(entries)}")
    for i, (n, s, o, t) in enumerate(entries):
        if names[i] != n:
            raise TrainStateError(f"train state: entry {i} is '{names[i]}', the model has '{n}' there")
        got = tuple(int(v) for v in shapes[i] if v >= 0)
        if got != tuple(s):
            raise TrainStateError(f"train state: wrong shape of '{n}': {got}, the model has {tuple(s)}")
    if not np.array_equal(z["entry_offsets"], want["entry_offsets"]) or not np.array_equal(z["entry_trainable"], want["entry_trainable"]):
        raise TrainStateError("train state: the parameter layout (offsets / trainable flags) is not the model's")
    n_total = sum(int(np.prod(s)) for _, s, _, _ in entries)
    n_train = sum(int(np.prod(s)) for _, s, _, t in entries if t)
    for k, n in zip(ARRAYS, (n_total, n_train, n_train, n_train)):
        a = z[k]
        if a.dtype != np.float32 or a.shape != (n,):
            raise TrainStateError(f"train state: wrong shape of '{k}': {a.dtype}{tuple(a.shape)}, expected float32({n},)")
    if int(z["accumulate_steps"]) < 1 or int(z["iterations"]) < 0 or int(z["steps"]) < 0:
        raise TrainStateError("train state: a counter is out of range")
    if "ema_avg" in keys:               # the moving average is optional: a file without it is a complete version-1 state
        for k in EMA_KEYS:
            if k not in keys:
                raise TrainStateError(f"train state: missing entry '{k}' (the file holds 'ema_avg')")
        a = z["ema_avg"]
        if a.dtype != np.float32 or a.shape != (n_train,):
            raise TrainStateError(f"train state: wrong shape of 'ema_avg': {a.dtype}{tuple(a.shape)}, expected float32({n_train},)")
        m = float(z["ema_momentum"])
        if int(z["ema_updates"]) < 0 or int(z["ema_overwrite_frequency"]) < 0 or not 0.0 <= m < 1.0:
            raise TrainStateError("train state: an entry of the moving average (ema_updates, ema_overwrite_frequency, ema_momentum) is out of range")
    if "awp_delta" in keys:             # so are the options of adversarial weight perturbation
        for k in AWP_KEYS:
            if k not in keys:
                raise TrainStateError(f"train state: missing entry '{k}' (the file holds 'awp_delta')")
        d, e = float(np.float32(z["awp_delta"])), float(np.float32(z["awp_eps"]))
        if not (math.isfinite(d) and d > 0 and math.isfinite(e) and e > 0 and int(z["awp_start_step"]) >= 0):
            raise TrainStateError("train state: an option of the weight perturbation (awp_delta, awp_eps, awp_start_step) is out of range")
    if "param_groups" in keys:          # and the optimizer's parameter groups
        try:
            resolve_param_groups(entries, json.loads(str(z["param_groups"])))
        except ValueError as e:
            raise TrainStateError(f"train state: the entry 'param_groups' does not fit the model: {e}")
    if "mwer" in keys:                  # and the options of minimum-risk training
        try:
            mwer_options(str(z["mwer"]))
        except (ValueError, TypeError) as e:
            raise TrainStateError(f"train state: the entry 'mwer' is not the seven mwer_* options: {e}")
    if "kd" in keys:                    # and the options of distillation
        try:
            kd_options(str(z["kd"]))
        except (ValueError, TypeError) as e:
            raise TrainStateError(f"train state: the entry 'kd' is not the five kd_* options: {e}")


def unpack_state(z, entries) -> dict:
    """validate_state, then plain Python values: the four arrays (float32, flat) and the scalars; global_clipnorm is None when off.  A file
    with the moving average adds ema_avg (float32), ema_updates, use_ema, ema_momentum, ema_warmup and ema_overwrite_frequency (None when
    off); a file without it adds none of them.  A file with the options of the weight perturbation adds awp_delta, awp_eps, awp_start_step
    and awp_relative; a file with the optimizer's parameter groups adds param_groups (the checked list); a file with the options of
    minimum-risk training adds mwer (the checked dict of the seven mwer_* options); a file with the options of distillation adds kd (the
    checked dict of the five kd_* options)."""
    validate_state(z, entries)
    out = {k: np.array(z[k], dtype=np.float32) for k in ARRAYS}
    for k in ("iterations", "steps", "step_seed", "accumulate_steps", "skipped"):
        out[k] = int(z[k])
    for k in ("learning_rate", "weight_decay"):
        out[k] = float(z[k])
    for k in ("apply_weight_decay", "skip_nonfinite"):
        out[k] = bool(z[k])
    clip = float(z["global_clipnorm"])
    out["global_clipnorm"] = clip if clip > 0 else None
    keys = set(z.files) if hasattr(z, "files") else set(z)
    if "ema_avg" in keys:
        every = int(z["ema_overwrite_frequency"])
        out.update(ema_avg=np.array(z["ema_avg"], dtype=np.float32), ema_updates=int(z["ema_updates"]), use_ema=bool(z["use_ema"]),
                   ema_momentum=float(z["ema_momentum"]), ema_warmup=bool(z["ema_warmup"]), ema_overwrite_frequency=every if every > 0 else None)
    if "awp_delta" in keys:
        out.update(awp_delta=float(z["awp_delta"]), awp_eps=float(z["awp_eps"]), awp_start_step=int(z["awp_start_step"]), awp_relative=bool(z["awp_relative"]))
    if "param_groups" in keys:
        out.update(param_groups=check_param_groups(json.loads(str(z["param_groups"]))))
    if "mwer" in keys:
        out.update(mwer=mwer_options(str(z["mwer"])))
    if "kd" in keys:
        out.update(kd=kd_options(str(z["kd"])))
    return out


def save_state_file(path: str, state: Dict[str, np.ndarray]) -> str:
    path = path if path.endswith(".npz") else path + ".npz"
    np.savez(path, **state)
    return path


def load_state_file(path: str, entries) -> dict:
    with np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False) as z:
        return unpack_state(z, entries)
