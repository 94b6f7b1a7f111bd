"""A plain-Python restatement of the merging WindowOperator / EvictingWindowOperator over EventTimeSessionWindows with
EventTimeTrigger or CountTrigger (each optionally inside PurgingTrigger): the checker of the GPU list operator's
CountTrigger over sessions and of its session snapshots (oracle/list_oracle.cpp refuses count sessions).  It is
ContinuousRef (tests/continuous_ref.py: MergingWindowSet.addWindow with HashSet order, the explicit timer set,
lateness, side output, evictors, emitWindowContents) with CountTrigger added (flink-streaming-java,
api/windowing/triggers/CountTrigger.java:47-85):
  onElement   count += 1 (a ReducingState "count" keyed by the actual window); at n the count is cleared and FIRE
  onEventTime CONTINUE (no timer is ever registered; the cleanup timer drops the window without a firing)
  onMerge     mergePartitionedState: the merged windows' counts summed under the merge result; no firing
  clear       the count is cleared
and session_state(): per key its in-flight windows as (actual window, state window, trigger state, list)."""
import numpy as np

from tests.continuous_ref import LMAX, LMIN, ContinuousRef, hashset_order  # noqa: F401


class SessionRef(ContinuousRef):
    def __init__(self, gap, trigger="event_time", trigger_count=0, interval=0, **kw):
        assert trigger in ("event_time", "count", "continuous")
        assert trigger != "count" or trigger_count >= 1
        # (ContinuousRef knows the two event-time triggers; the count trigger's four callbacks are overridden below)
        super().__init__(assigner="session", gap=gap, trigger="event_time" if trigger == "count" else trigger,
                         interval=interval, **kw)
        self.trigger, self.trigger_count = trigger, trigger_count
        self.count = {}  # (key, window) -> CountTrigger's "count", absent = null
        self.count_merges = 0     # merges that summed at least two non-null counts
        self.fired_after_merge = 0  # firings of a window whose merged counts alone had reached n

    def _on_element(self, ts, key, w):
        if self.trigger != "count":
            return super()._on_element(ts, key, w)
        c = self.count.get((key, w), 0) + 1
        if c >= self.trigger_count:
            if c - 1 >= self.trigger_count:
                self.fired_after_merge += 1
            self.count.pop((key, w), None)
            return True
        self.count[(key, w)] = c
        return False

    def _on_event_time(self, t, key, w):
        return False if self.trigger == "count" else super()._on_event_time(t, key, w)

    def _trigger_clear(self, key, w):
        if self.trigger == "count":
            self.count.pop((key, w), None)
        else:
            super()._trigger_clear(key, w)

    def _trigger_on_merge(self, key, result, merged, target_window):
        if self.trigger != "count":
            return super()._trigger_on_merge(key, result, merged, target_window)
        parts = [self.count.pop((key, m)) for m in merged if (key, m) in self.count]
        if parts:
            self.count[(key, result)] = self.count.get((key, result), 0) + sum(parts)
            self.count_merges += len(parts) > 1

    def load_state(self, rows):
        """initializeState from rows [(key, start, end, state start, state end, count, values)] of a
        CountTrigger savepoint: the mapping, the lists, the counts and every window's cleanup timer; restored
        elements carry no timestamp and are numbered first"""
        assert self.trigger == "count"
        for key, s, e, ss, se, cnt, values in rows:
            self.mapping.setdefault(key, {})[(s, e)] = (ss, se)
            if values:
                lst = self.state.setdefault((key, (ss, se)), [])
                for v in values:
                    lst.append((LMIN, v, self.ordinal))
                    self.ordinal += 1
            if cnt:
                self.count[(key, (s, e))] = cnt
            self._register(self._cleanup_time((s, e)), key, (s, e))

    def session_state(self):
        """{key: sorted [(start, end, state start, state end, trigger state, timer bits, ((ts, val, ordinal), ...))]}:
        the trigger state is the count (CountTrigger), the fire time or Long.MIN_VALUE (ContinuousEventTimeTrigger),
        else 0; timer bit 1 = the maxTimestamp timer is registered, 2 = the timer at the fire time"""
        out = {}
        for key, mapping in self.mapping.items():
            rows = []
            for w, sw in mapping.items():
                if self.trigger == "count":
                    ts, bits = self.count.get((key, w), 0), 0
                elif self.trigger == "continuous":
                    ts = self.fire.get((key, w), LMIN)
                    bits = int((self._max_ts(w), key, w) in self.timers) | 2 * int((ts, key, w) in self.timers)
                else:
                    ts, bits = 0, int((self._max_ts(w), key, w) in self.timers)
                rows.append((w[0], w[1], sw[0], sw[1], ts, bits, tuple(self.state.get((key, sw), ()))))
            out[key] = sorted(rows)
        return out


def gpu_state(snapshot):
    """the same form from a GPU handle's {key group: (windows SESSION_STATE_DTYPE, elements)}"""
    out = {}
    for wins, el in snapshot.values():
        o = 0
        for r in wins:
            n = int(r["n_elems"])
            lst = tuple((int(e["ts"]), int(e["val"]), int(e["ordinal"])) for e in el[o:o + n])
            o += n
            out.setdefault(int(r["key"]), []).append((int(r["start"]), int(r["end"]), int(r["state_start"]),
                                                      int(r["state_end"]), int(r["trigger_state"]), int(r["timer"]), lst))
        assert o == len(el)
    return {k: sorted(v) for k, v in out.items()}


def load_session_kats():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "session_count_kats.json")) as f:
        return json.load(f)["cases"]


def session_stream(seed, n, keys, span, jitter, zipf=False):
    """seeded (key, ts, i64 value) columns: timestamps advance over `span` with `jitter` of disorder, so elements open
    sessions, extend them, arrive behind them and bridge two of them"""
    rng = np.random.default_rng(seed)
    if zipf:
        w = 1.0 / np.arange(1, keys + 1) ** 1.1
        k = rng.choice(keys, n, p=w / w.sum()).astype(np.int64) * 7919 + 13
    else:
        k = rng.integers(0, keys, n, dtype=np.int64)
    t = np.arange(n, dtype=np.int64) * span // n - rng.integers(0, jitter, n, dtype=np.int64)
    v = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    return k, t, v
