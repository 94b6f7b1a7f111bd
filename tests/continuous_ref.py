"""A plain-Python restatement of WindowOperator / EvictingWindowOperator over ListState with an explicit timer set and
a pluggable trigger (EventTimeTrigger, ContinuousEventTimeTrigger, each optionally inside PurgingTrigger): the
checker of the GPU list operator's ContinuousEventTimeTrigger.  Slow and obvious on purpose: one record at a time,
one timer at a time.  Sources (flink-streaming-java, org/apache/flink/streaming/):
  runtime/operators/windowing/WindowOperator.java:291-469 processElement / onEventTime, :576-651 lateness, cleanup
  runtime/operators/windowing/EvictingWindowOperator.java:102-286, :334-380 emitWindowContents / clearAllState
  runtime/operators/windowing/MergingWindowSet.java:150-225 addWindow; api/windowing/windows/TimeWindow.java:201-244
  api/windowing/triggers/{EventTimeTrigger.java:37-73, ContinuousEventTimeTrigger.java:39-151, PurgingTrigger.java}
  api/windowing/evictors/{CountEvictor.java:50-78, TimeEvictor.java:54-104}
  api/operators/HeapInternalTimerService.java advanceWatermark: timers <= the watermark, in ascending time, those
  registered on the way included.
The interface is ListWindowOracle's (oracle/oracle.py): process, watermark, contents, side_rows, late_dropped,
num_state_entries, num_timers."""
import heapq
import struct

import numpy as np

LMIN, LMAX = -(1 << 63), (1 << 63) - 1
ROW_DTYPE = np.dtype([(f, "<i8") for f in ("key", "start", "end", "count", "sum", "min", "max", "first", "elem_off",
                                          "epoch")])
ELEM_DTYPE = np.dtype([("ts", "<i8"), ("val", "<i8"), ("ordinal", "<i8")])


def jwrap(x):
    """a Java long: two's complement wrap"""
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def jrem(a, b):
    """Java's %: the remainder takes the dividend's sign"""
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def _f64(bits):
    return struct.unpack("<d", struct.pack("<q", bits))[0]


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _dkey(bits):
    """Double.compare's order of a double's bits"""
    return bits if bits >= 0 else bits ^ 0x7fffffffffffffff


def hashset_order(windows):
    """the iteration order of a java.util.HashSet<TimeWindow> of capacity 16 filled in the given order:
    TimeWindow.hashCode = MathUtils.longToIntWithBitMixing(start + end) (TimeWindow.java:102-104, MathUtils.java
    :177-182), HashMap's spread h ^ (h >>> 16), bucket = spread & 15; buckets ascending, a bucket in insertion order"""
    def bucket(w):
        m = (1 << 64) - 1
        x = (w[0] + w[1]) & m
        x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & m
        x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & m
        h = (x ^ (x >> 31)) & 0xffffffff
        return (h ^ (h >> 16)) & 15
    return [w for _, _, w in sorted((bucket(w), i, w) for i, w in enumerate(windows))]


class TimerRunaway(RuntimeError):
    """the reference would not return in any useful time on this stream (ContinuousRef timer_cap, the sliding walk)"""


class ContinuousRef:
    def __init__(self, assigner="tumbling", size=0, slide=0, offset=0, gap=0, lateness=0, trigger="event_time",
                 interval=0, purging=False, evictor="none", evict_after=False, evict_arg=0, side_output=False,
                 value_type="i64", timer_cap=None):
        assert assigner in ("tumbling", "sliding", "global", "session")
        assert trigger in ("event_time", "continuous") and evictor in ("none", "count", "time")
        assert value_type in ("i64", "f64") and (trigger != "continuous" or interval >= 1)
        self.assigner, self.size, self.slide, self.offset, self.gap = assigner, size, slide, offset, gap
        self.lateness, self.trigger, self.interval, self.purging = lateness, trigger, interval, purging
        self.evictor, self.evict_after, self.evict_arg = evictor, evict_after, evict_arg
        self.side_output, self.value_type = side_output, value_type
        # the most timers one watermark may fire (None: no bound).  A ContinuousEventTimeTrigger whose first timer
        # ts - ts % interval + interval wraps past Long.MAX_VALUE starts its chain at the bottom of the range, and
        # unless the window's cleanup timer comes first the chain walks up to the watermark, 2^64 / interval steps in
        # the reference too: TimerRunaway instead of not returning
        self.timer_cap = timer_cap
        self.wm = LMIN
        self.epoch = 0
        self.ordinal = 0
        self.late_dropped = 0
        self.timers = set()       # (time, key, window): HeapInternalTimerService's event-time timers
        self.heap = []            # the same, ordered (entries no longer in the set are skipped)
        self.state = {}           # (key, state window) -> [(ts, val, ordinal)], absent = null
        self.fire = {}            # (key, window) -> ContinuousEventTimeTrigger's "fire-time"
        self.mapping = {}         # key -> {window: state window} (MergingWindowSet)
        self._rows, self._elems, self._side = [], [], []
        self.merges = 0           # merge function calls
        self.fire_from_other = 0  # merges whose fire time came from a window other than the merge target's
        self.early_by_window = {}  # (key, window) -> firings at timers other than maxTimestamp
        self.stuck_windows = set()  # (key, window) that fired at maxTimestamp with fire == maxTimestamp

    # ------------------------------------------------------------------ windows
    def _event_time(self):
        return self.assigner != "global"

    def _assign(self, ts):
        if self.assigner == "global":
            return [(LMIN, LMAX)]
        if self.assigner == "session":
            return [(ts, jwrap(ts + self.gap))]
        if self.assigner == "tumbling":
            s = jwrap(ts - jrem(jwrap(jwrap(ts - self.offset) + self.size), self.size))
            return [(s, jwrap(s + self.size))]
        last = jwrap(ts - jrem(jwrap(jwrap(ts - self.offset) + self.slide), self.slide))
        out, s = [], last
        while s > jwrap(ts - self.size):
            if len(out) == -(-self.size // self.slide) + 1:  # (the walk wrapped below Long.MIN_VALUE: window_ref.Runaway)
                raise TimerRunaway(f"sliding walk of ts {ts} does not end")
            out.append((s, jwrap(s + self.size)))
            s = jwrap(s - self.slide)
        return out

    def _max_ts(self, w):
        return LMAX if self.assigner == "global" else jwrap(w[1] - 1)

    def _cleanup_time(self, w):  # WindowOperator.cleanupTime
        if not self._event_time():
            return self._max_ts(w)
        t = jwrap(self._max_ts(w) + self.lateness)
        return t if t >= self._max_ts(w) else LMAX

    def _window_late(self, w):
        return self._event_time() and self._cleanup_time(w) <= self.wm

    # ------------------------------------------------------------------ timers
    def _register(self, t, key, w):
        if (t, key, w) not in self.timers:
            self.timers.add((t, key, w))
            heapq.heappush(self.heap, (t, key, w))

    def _delete(self, t, key, w):
        self.timers.discard((t, key, w))

    # ------------------------------------------------------------------ the trigger
    def _on_element(self, ts, key, w):
        """True = FIRE"""
        if self._max_ts(w) <= self.wm:
            return True
        self._register(self._max_ts(w), key, w)
        if self.trigger == "continuous" and (key, w) not in self.fire:
            nxt = jwrap(jwrap(ts - jrem(ts, self.interval)) + self.interval)
            self._register(nxt, key, w)
            self.fire[(key, w)] = nxt
        return False

    def _on_event_time(self, t, key, w):
        if t == self._max_ts(w):
            if self.fire.get((key, w)) == t:
                self.stuck_windows.add((key, w))
            return True
        if self.trigger == "continuous" and self.fire.get((key, w)) == t:
            self.fire[(key, w)] = jwrap(t + self.interval)
            self._register(jwrap(t + self.interval), key, w)
            self.early_by_window[(key, w)] = self.early_by_window.get((key, w), 0) + 1
            return True
        return False

    def _trigger_clear(self, key, w):
        if self.trigger == "continuous":
            f = self.fire.pop((key, w), None)
            if f is not None:
                self._delete(f, key, w)
        else:
            self._delete(self._max_ts(w), key, w)

    def _trigger_on_merge(self, key, result, merged, target_window):
        if self.trigger == "continuous":  # mergePartitionedState: Min over the merged windows' fire times
            fires = [(self.fire.pop((key, m)), m) for m in merged if (key, m) in self.fire]
            if fires:
                f = min(x for x, _ in fires)
                self.fire[(key, result)] = f
                tf = [x for x, m in fires if m == target_window]
                if not tf or tf[0] > f:
                    self.fire_from_other += 1
                self._register(f, key, result)
        else:
            self._register(self._max_ts(result), key, result)

    # ------------------------------------------------------------------ evictors and the firing
    def _evict(self, lst):
        size = len(lst)
        if self.evictor == "count":
            if size > self.evict_arg:
                del lst[:size - self.evict_arg]
        elif self.evictor == "time" and lst and lst[0][0] != LMIN:
            cutoff = jwrap(max(e[0] for e in lst) - self.evict_arg)
            lst[:] = [e for e in lst if not e[0] <= cutoff]

    def _emit(self, key, w, sk):
        lst = self.state[sk]
        if self.evictor != "none" and not self.evict_after:
            self._evict(lst)
        seen = list(lst)
        if self.value_type == "f64":
            s = 0.0
            for i, e in enumerate(seen):
                s = _f64(e[1]) if i == 0 else s + _f64(e[1])
            total = _bits(s)
            mn = min((e[1] for e in seen), key=_dkey, default=0)
            mx = max((e[1] for e in seen), key=_dkey, default=0)
        else:
            total = 0
            for e in seen:
                total = jwrap(total + e[1])
            mn = min((e[1] for e in seen), default=0)
            mx = max((e[1] for e in seen), default=0)
        self._rows.append((key, w[0], w[1], len(seen), total, mn, mx, seen[0][2] if seen else -1, len(self._elems),
                           self.epoch))
        self._elems.extend(seen)
        if self.evictor != "none":
            if self.evict_after:
                self._evict(lst)
            if not lst:  # windowState.clear() and nothing added back: the state is null
                del self.state[sk]

    def _clear_all(self, key, w, sk):
        self.state.pop(sk, None)
        self._trigger_clear(key, w)
        if self.assigner == "session":
            self.mapping[key].pop(w, None)
            if not self.mapping[key]:
                del self.mapping[key]

    # ------------------------------------------------------------------ MergingWindowSet.addWindow
    def _add_window(self, key, new):
        mapping = self.mapping.setdefault(key, {})
        windows = sorted(list(mapping) + [new], key=lambda w: w[0])  # (stable: the new window after an equal start)
        merged = []  # TimeWindow.mergeWindows
        for w in windows:
            if merged and merged[-1][0][0] <= w[1] and merged[-1][0][1] >= w[0]:
                c = merged[-1][0]
                merged[-1][0] = (min(c[0], w[0]), max(c[1], w[1]))
                if w not in merged[-1][1]:  # (a HashSet: an equal window is already in it)
                    merged[-1][1].append(w)
            else:
                merged.append([w, [w]])
        result_window = new
        for res, members in merged:
            if len(members) < 2:
                continue
            members = hashset_order(members)
            if new in members:
                members.remove(new)
                result_window = res
            target_state = mapping[members[0]]
            merged_states = [mapping.pop(m) for m in members]
            mapping[res] = target_state
            merged_states.remove(target_state)
            if res in members and len(members) == 1:
                continue
            # the merge function (WindowOperator.java:308-339)
            if self._max_ts(res) + self.lateness <= self.wm:
                raise RuntimeError("The end timestamp of an event-time window cannot become earlier than the current "
                                   "watermark by merging.")
            self.merges += 1
            self._trigger_on_merge(key, res, members, members[0])
            for m in members:
                self._trigger_clear(key, m)
                self._delete(self._cleanup_time(m), key, m)
            lst = None  # mergeNamespaces: the sources in order, then behind the target's own list
            for s in merged_states:
                src = self.state.pop((key, s), None)
                if src is not None:
                    lst = src if lst is None else lst + src
            if lst is not None:
                self.state[(key, target_state)] = self.state.get((key, target_state), []) + lst
        if new not in mapping and result_window == new:
            mapping[new] = new
        return result_window

    # ------------------------------------------------------------------ processElement / processWatermark
    def _element(self, key, ts, val):
        o = self.ordinal
        self.ordinal += 1
        skipped = True
        for w in self._assign(ts):
            if self.assigner == "session":
                w = self._add_window(key, w)
                if self._window_late(w):
                    self.mapping[key].pop(w, None)  # retireWindow
                    if not self.mapping[key]:
                        del self.mapping[key]
                    continue
                sk = (key, self.mapping[key][w])
            else:
                if self._window_late(w):
                    continue
                sk = (key, w)
            skipped = False
            self.state.setdefault(sk, []).append((ts, val, o))
            if self._on_element(ts, key, w):
                self._emit(key, w, sk)
                if self.purging:
                    self.state.pop(sk, None)
            ct = self._cleanup_time(w)  # registerCleanupTimer
            if ct != LMAX:
                self._register(ct, key, w)
        if skipped and self._event_time() and jwrap(ts + self.lateness) <= self.wm:
            if self.side_output:
                self._side.append((self.epoch, key, ts, val))
            else:
                self.late_dropped += 1

    def process(self, keys, ts, vals):
        vals = np.asarray(vals)
        if vals.dtype == np.float64:
            vals = vals.view(np.int64)
        for k, t, v in zip(np.asarray(keys).tolist(), np.asarray(ts).tolist(), vals.tolist()):
            self._element(k, t, v)

    def watermark(self, wm):
        wm = int(wm)
        if wm > self.wm:
            self.wm = wm
            fired = 0
            while self.heap and self.heap[0][0] <= wm:
                t, key, w = heapq.heappop(self.heap)
                if (t, key, w) not in self.timers:
                    continue
                fired += 1
                if self.timer_cap is not None and fired > self.timer_cap:
                    raise TimerRunaway(f"watermark {wm} fires more than {self.timer_cap} timers")
                self.timers.discard((t, key, w))
                self._timer(t, key, w)
        self.epoch += 1

    def _timer(self, t, key, w):  # onEventTime
        if self.assigner == "session":
            sw = self.mapping.get(key, {}).get(w)
            if sw is None:
                return  # a timer of a window that is gone
            sk = (key, sw)
        else:
            sk = (key, w)
        if sk in self.state:  # contents != null
            if self._on_event_time(t, key, w):
                self._emit(key, w, sk)
                if self.purging:
                    self.state.pop(sk, None)
        if self._event_time() and t == self._cleanup_time(w):
            self._clear_all(key, w, sk)

    # ------------------------------------------------------------------ results
    def rows(self):
        return np.array(self._rows, dtype=ROW_DTYPE) if self._rows else np.zeros(0, dtype=ROW_DTYPE)

    def contents(self):
        e = np.array(self._elems, dtype=ELEM_DTYPE) if self._elems else np.zeros(0, dtype=ELEM_DTYPE)
        return [(r, e[r["elem_off"]:r["elem_off"] + r["count"]]) for r in self.rows()]

    def side_rows(self):
        a = np.array(self._side, dtype=np.int64).reshape(-1, 4)
        return [a[:, i].copy() for i in range(4)]

    @property
    def num_state_entries(self):
        return len(self.state)

    @property
    def num_timers(self):
        return len(self.timers)

    def close(self):
        pass


# ---------------------------------------------------------------- the known-answer sequences
def load_continuous_kats():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "continuous_trigger_kats.json")) as f:
        return json.load(f)["cases"]


def replay_kat(case, op):
    """[(rows the step produced, rows the step expects)] as sorted (key, start, end, count, sum) lists; op is a
    ContinuousRef or a GpuListWindowOperator (rows() grows with every firing)"""
    lim = {"MIN": LMIN, "MAX": LMAX}
    out, seen = [], 0
    for step in case["steps"]:
        if "elements" in step:
            k, t, v = (np.array(c, dtype=np.int64) for c in zip(*step["elements"]))
            op.process(k, t, v)
        else:
            op.watermark(step["watermark"])
        rows = op.rows()
        got = sorted((int(r["key"]), int(r["start"]), int(r["end"]), int(r["count"]), int(r["sum"]))
                     for r in rows[seen:])
        seen = len(rows)
        out.append((got, sorted(tuple(lim.get(x, x) for x in r) for r in step.get("rows", []))))
    return out


# ---------------------------------------------------------------- the seeded configurations (CPU and GPU tests)
# Non-merging windows over the stream _stream(seed, 20000, 37, 2000, 150) of tests/test_gpu_list.py.  Fire times are
# multiples of the interval, a tumbling window [100 k, 100 k + 100) has maxTimestamp 100 k + 99: with interval 11
# the windows k = 0 and 11 meet it (100 k + 99 = k mod 11) and stop there, the others fire about nine times early;
# with interval 250 only the windows that hold a multiple of 250 fire early at all; with interval 33 a sliding window
# [25 j, 25 j + 100) meets its maxTimestamp for j = 0, 33, 66.
NONMERGING_CONFIGS = [
    dict(assigner="tumbling", size=100, interval=11),
    dict(assigner="tumbling", size=100, lateness=50, purging=True, side_output=True, interval=33),
    dict(assigner="sliding", size=100, slide=25, lateness=40, interval=33),
    dict(assigner="tumbling", size=100, evictor="count", evict_arg=3, interval=11),
    dict(assigner="tumbling", size=100, evictor="count", evict_arg=2, evict_after=True, lateness=30, interval=250),
    dict(assigner="tumbling", size=200, evictor="time", evict_arg=50, interval=40),
    dict(assigner="global", interval=100),
]
SESSION_CONFIGS = [
    dict(assigner="session", gap=30, interval=20),
    dict(assigner="session", gap=30, lateness=200, interval=60),
    dict(assigner="session", gap=30, lateness=200, purging=True, side_output=True, interval=45),
    dict(assigner="session", gap=30, evictor="count", evict_arg=3, interval=20),
]


def seeded_stream(seed, n, keys, span, jitter):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, keys, n, dtype=np.int64)
    t = np.arange(n, dtype=np.int64) * span // n - rng.integers(0, jitter, n, dtype=np.int64)
    v = rng.integers(-1000, 1000, n, dtype=np.int64)
    return k, t, v


def zipf_stream(seed, n, keys, span, jitter, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, keys + 1) ** s
    k = rng.choice(keys, n, p=w / w.sum()).astype(np.int64) * 7919 + 13
    t = np.arange(n, dtype=np.int64) * span // n - rng.integers(0, jitter, n, dtype=np.int64)
    v = rng.integers(-1000, 1000, n, dtype=np.int64)
    return k, t, v


def drive(ops, k, t, v, batches=10, bound=100, final=(500, "max"), each=None):
    """the seeded tests' schedule: `batches` pushes, a watermark `bound` behind the newest timestamp after two of
    every three, then a jump by final[0] and (final[1] == "max") to Long.MAX_VALUE; each(): after every step"""
    n = len(k) // batches
    wm = -10**9
    for b in range(batches):
        sl = slice(b * n, (b + 1) * n)
        for h in ops:
            h.process(k[sl], t[sl], v[sl].view(np.float64) if getattr(h, "wants_f64", False) else v[sl])
        wm = max(wm, int(t[sl].max()) - bound)
        if b % 3 != 1:
            for h in ops:
                h.watermark(wm)
        if each:
            each()
    for w in [wm + final[0]] + ([LMAX] if final[1] == "max" else []):
        for h in ops:
            h.watermark(w)
