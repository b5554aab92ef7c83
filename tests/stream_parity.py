"""Case tables and helpers of the streaming tests (test_stream.py, test_stream_mutants.py, test_stream_gpu.py).

A scenario is a fixed, seeded list of ticks.  `run_append` / `run_agree` drive a StreamReference (or a mutant of it) through one and return a
snapshot of every array the device writes after every tick; the GPU tests build the same snapshots from the device and compare them with
`mismatches`, the comparison the mutant tests prove sharp."""
import numpy as np

from ishara_amd import tflite_stream as TS
from ishara_amd.tflite_stream import C_ACTIVE, C_CLEN, C_NHIST, FINISH, RESET, StreamReference

N_COLS = 276
SENTINEL = np.float32(-12345.5)        # pre-fill of the session rows: what the append must not touch


# ---------------------------------------------------------------------------------------------------- frames
def frames(k, seed, hand=0.5, lead_silence=0):
    """k raw frames: Gaussian landmarks, the three hand blocks of a frame all NaN with probability 1 - hand (as in real clips, and always in
    the first lead_silence frames), scattered NaNs elsewhere."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((k, N_COLS)).astype(np.float32)
    for f in range(k):
        if f < lead_silence or g.random() >= hand:
            for a in range(3):
                x[f, a * 92: a * 92 + 42] = np.nan
        if g.random() < 0.1:
            x[f, g.integers(0, N_COLS, 5)] = np.nan
    return x


def cancelling_frame(seed=0):
    """A frame whose hand values are finite but sum to exactly 0 in float32: the filter calls it hand-less."""
    x = frames(1, seed, hand=0.0)[0]
    x[3], x[92 + 7] = np.float32(0.625), np.float32(-0.625)
    return x


# ---------------------------------------------------------------------------------------------------- comparison
def mismatches(got, want):
    """Names (with the tick) of the arrays that differ between two snapshot lists; floats are compared as bit patterns."""
    bad = []
    assert len(got) == len(want)
    for t, (a, b) in enumerate(zip(got, want)):
        assert a.keys() == b.keys()
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            if x.dtype == np.float32:
                x, y = x.view(np.uint32), y.view(np.uint32)
            if x.shape != y.shape or not np.array_equal(x, y):
                bad.append((t, k))
    return bad


# ---------------------------------------------------------------------------------------------------- append scenario
APPEND = dict(S=5, window=70, T=24)
APPEND_LENGTHS = (0, 1, 9, 64, 65, 130, 200, 300)      # 300: a second round of the kernel's 256-frame ballots; 200, 300 > window


def append_ticks():
    """[(chunks [S], flags [S])]: every chunk length on a session that has not started, on one in the middle of a phrase and on a full one,
    leading silence longer than a ballot round, a cancelling frame as the only 'hand' of a chunk, resets."""
    S = APPEND["S"]
    g = np.random.default_rng(70)
    ticks = []
    # tick 0: silence past the first ballot round (first hand at 270 of 300), a hand at index 0 / in the middle / at the last index / nowhere
    first = [frames(300, 1, hand=0.6, lead_silence=270), frames(9, 2, hand=1.0), frames(9, 3, hand=0.0), frames(9, 4, hand=0.0), frames(9, 5, hand=0.0)]
    first[2][4] = frames(1, 6, hand=1.0)[0]
    first[3][8] = frames(1, 7, hand=1.0)[0]
    first[4][5] = cancelling_frame()                   # still no hand: the session does not start
    ticks.append((first, np.zeros(S, np.int32)))
    for t in range(1, 11):
        lens = g.choice(APPEND_LENGTHS, S)
        chunks = [frames(int(k), 100 * t + s, hand=0.35, lead_silence=int(g.integers(0, 3))) for s, k in enumerate(lens)]
        flags = np.where(g.random(S) < 0.2, RESET, 0).astype(np.int32)
        if t == 1:
            flags[0] = RESET                           # the full session 0 starts again, with a chunk whose only non-NaN hand cancels
            chunks[0] = frames(9, 50, hand=0.0)
            chunks[0][2] = cancelling_frame(1)
            chunks[4] = np.concatenate([frames(3, 51, hand=0.0), cancelling_frame(2)[None], frames(5, 52, hand=1.0)])
        ticks.append((chunks, flags))
    return ticks


def append_snapshot(raw, hand, counters, fresh):
    return dict(raw=np.array(raw, np.float32), hand=np.array(hand, np.uint8), counters=np.array(counters, np.int32), fresh=np.array(fresh, np.int32))


def new_append_reference(cls=StreamReference):
    ref = cls(APPEND["S"], APPEND["window"], APPEND["T"])
    ref.raw[:] = SENTINEL
    ref.hand[:] = 0xEE
    return ref


def run_append(ref, ticks):
    snaps = []
    for chunks, flags in ticks:
        fresh = np.zeros(ref.S, np.int32)
        for s in range(ref.S):
            ref.start(s, int(flags[s]))
            fresh[s] = ref.append(s, chunks[s])
        snaps.append(append_snapshot(ref.raw, ref.hand, ref.counters, fresh))
    return snaps


# ---------------------------------------------------------------------------------------------------- agree scenario
AGREE = dict(S=8, window=70, T=12, idle_frames=4, min_active_frames=3, ticks=200)
AGREE_SEED = 5


def agree_ticks(seed=AGREE_SEED):
    """[(idx [S, T], len [S], fresh [S], flags [S], cnt [S, 4])]: per session a hypothesis that grows, is revised in place, shrinks or stays
    (lengths 0..T), a tick in four not fresh, rare FINISH / RESET, and synthetic n / active / idle / dropped counters (set in front of the
    agree step: this scenario has no frames) whose idle run reaches the endpoint now and then."""
    S, T = AGREE["S"], AGREE["T"]
    g = np.random.default_rng(seed)
    hyp = [[] for _ in range(S)]
    cnt = np.zeros((S, 4), np.int32)
    ticks = []
    for _ in range(AGREE["ticks"]):
        idx, ln = np.full((S, T), -1, np.int32), np.zeros(S, np.int32)
        fresh = (g.random(S) < 0.75).astype(np.int32)
        flags = np.zeros(S, np.int32)
        u = g.random(S)
        flags[u < 0.03] = FINISH
        flags[(u >= 0.03) & (u < 0.05)] = RESET
        for s in range(S):
            if flags[s] & RESET:
                hyp[s], cnt[s] = [], 0
            r = g.random()
            if r < 0.45:
                hyp[s] = (hyp[s] + [int(g.integers(0, 59))])[:T]
            elif r < 0.60 and hyp[s]:
                hyp[s][int(g.integers(0, len(hyp[s])))] = int(g.integers(0, 59))
            elif r < 0.70:
                hyp[s] = hyp[s][:max(len(hyp[s]) - int(g.integers(1, 3)), 0)]
            elif r < 0.72:
                hyp[s] = [int(v) for v in g.integers(0, 59, T)]                # len = T
            ln[s] = len(hyp[s])
            idx[s, :ln[s]] = hyp[s]
            if fresh[s]:
                if g.random() < 0.8:
                    cnt[s, 0], cnt[s, 1], cnt[s, 2] = cnt[s, 0] + 1, cnt[s, 1] + 1, 0
                else:
                    cnt[s, 0], cnt[s, 2] = cnt[s, 0] + 1, cnt[s, 2] + 1
                cnt[s, 0] = min(cnt[s, 0], AGREE["window"])
        ticks.append((idx, ln, fresh, flags, cnt.copy()))
        for s in range(S):                                                     # what ends a phrase here restarts the synthetic counters
            if (flags[s] & FINISH) or cnt[s, 0] >= AGREE["window"] or (cnt[s, 1] >= AGREE["min_active_frames"] and cnt[s, 2] >= AGREE["idle_frames"]):
                hyp[s], cnt[s] = [], 0
    return ticks


def agree_snapshot(record, text, counters, hist, hist_len, committed):
    return dict(record=np.array(record, np.int32), text=np.array(text, np.int32), counters=np.array(counters, np.int32),
                hist=np.array(hist, np.int32), hist_len=np.array(hist_len, np.int32), committed=np.array(committed, np.int32))


def new_agree_reference(A, cls=StreamReference):
    return cls(AGREE["S"], AGREE["window"], AGREE["T"], agree=A, idle_frames=AGREE["idle_frames"], min_active_frames=AGREE["min_active_frames"])


def run_agree(ref, ticks):
    """Snapshots per tick, and what the scenario exercised: sessions whose committed_len grew, attempts to retract (a hypothesis that
    contradicts or undercuts the committed prefix while the history is full), non-fresh ticks."""
    snaps, grew, stats = [], set(), dict(retractions=0, non_fresh=0)
    for idx, ln, fresh, flags, cnt in ticks:
        records, texts = np.zeros((ref.S, 8), np.int32), np.zeros((ref.S, ref.T), np.int32)
        for s in range(ref.S):
            ref.start(s, int(flags[s]))
            ref.counters[s, :4] = cnt[s]
            before = int(ref.counters[s, C_CLEN])
            hyp = idx[s, :ln[s]]
            records[s], texts[s] = ref.agree(s, hyp, bool(fresh[s]), int(flags[s]))
            after = int(ref.counters[s, C_CLEN])
            if after > before:
                grew.add(s)
            if ref.counters[s, C_NHIST] == ref.A and before > 0 and (ln[s] < before or not np.array_equal(hyp[:before], ref.committed[s, :before])):
                stats["retractions"] += 1
            stats["non_fresh"] += int(not fresh[s])
        snaps.append(agree_snapshot(records, texts, ref.counters, ref.hist, ref.hist_len, ref.committed))
    stats["sessions_grew"] = len(grew)
    return snaps, stats


# ---------------------------------------------------------------------------------------------------- mutants of the reference
class HistoryPushedWhenNotFresh(StreamReference):
    def agree(self, s, hyp, fresh, flags):
        rec, text = super().agree(s, hyp, True, flags)
        if not fresh:
            rec[0] &= ~TS.FRESH
        return rec, text


class PrefixOverAllButOne(StreamReference):
    def common_prefix(self, s):
        l, lens = 0, self.hist_len[s, 1:]
        while l < lens.min() and (self.hist[s, 1:, l] == self.hist[s, 1, l]).all():
            l += 1
        return l


class CommittedRewritten(StreamReference):
    def commit(self, s, hyp, l):
        c = self.counters[s]
        k = min(int(c[C_CLEN]), len(hyp))
        self.committed[s, :k] = hyp[:k]
        super().commit(s, hyp, l)


class IdleOffByOne(StreamReference):
    def append_frame(self, s, frame, hand):
        first_idle = not hand and self.counters[s, TS.C_IDLE] == 0 and self.counters[s, C_ACTIVE] > 0
        stored = super().append_frame(s, frame, hand)
        if stored and first_idle:
            self.counters[s, TS.C_IDLE] -= 1       # the run starts counting at its second frame
        return stored


class DroppedCountedAsStored(StreamReference):
    def append_frame(self, s, frame, hand):
        stored = super().append_frame(s, frame, hand)
        if not stored and self.counters[s, TS.C_N] < self.window:
            self.counters[s, TS.C_N] += 1
            self.counters[s, TS.C_DROPPED] -= 1
        return stored


class LeadingSilenceStored(StreamReference):
    def append_frame(self, s, frame, hand):
        c = self.counters[s]
        if c[C_ACTIVE] == 0 and not hand and c[TS.C_N] < self.window:
            n = int(c[TS.C_N])
            self.raw[s, n], self.hand[s, n] = frame, 0
            c[TS.C_N] += 1
            c[TS.C_IDLE] += 1
            return True
        return super().append_frame(s, frame, hand)


class ResetAfterFinalSkipped(StreamReference):
    def start(self, s, flags):
        if flags & RESET:
            self.counters[s] = 0
        self.counters[s, TS.C_DONE] = 0


MUTANTS = {
    "history_pushed_when_not_fresh": (HistoryPushedWhenNotFresh, "agree"),
    "prefix_over_all_but_one": (PrefixOverAllButOne, "agree"),
    "committed_rewritten": (CommittedRewritten, "agree"),
    "idle_off_by_one": (IdleOffByOne, "append"),
    "dropped_counted_as_stored": (DroppedCountedAsStored, "append"),
    "leading_silence_stored": (LeadingSilenceStored, "append"),
    "reset_after_final_skipped": (ResetAfterFinalSkipped, "agree"),
}
