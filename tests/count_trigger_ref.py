"""CountTrigger over time windows with an aggregating state, restated in plain Python for what the pinned
ListWindowOracle cannot express (restored trigger counts, counts >= n).  One dict entry per (key, window):
[count, sum, min, max, trigger_count].  Every rule cites the reference (paths under flink-streaming-java/src/main/java/
org/apache/flink/streaming/): WO = runtime/operators/windowing/WindowOperator.java, CT = api/windowing/triggers/
CountTrigger.java, PT = api/windowing/triggers/PurgingTrigger.java."""
import struct

LMAX = (1 << 63) - 1
LMIN = -(1 << 63)


def jrem(a, b):
    """Java's a % b for b > 0: the sign of the dividend (TimeWindow.getWindowStartWithOffset, TimeWindow.java:254-256)"""
    r = abs(a) % b
    return -r if a < 0 else r


def wrap32(x):
    return (int(x) + (1 << 31)) % (1 << 32) - (1 << 31)


def _f(bits):
    return struct.unpack("<d", struct.pack("<q", int(bits)))[0]


def _b(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


class CountTriggerRef:
    def __init__(self, assigner="tumbling", size=0, slide=0, offset=0, lateness=0, n=1, purging=False,
                 side_output=False, value_type="long"):
        self.assigner, self.size, self.slide, self.offset = assigner, size, slide or size, offset
        self.lateness, self.n, self.purging, self.side_output = lateness, n, purging, side_output
        self.value_type = value_type
        self.wm, self.epoch = LMIN, 0
        self.state = {}
        self._rows, self._side, self.late_dropped = [], [], 0

    def _windows(self, ts):
        if self.assigner == "tumbling":  # TumblingEventTimeWindows.java:64-68
            return [ts - jrem(ts - self.offset + self.size, self.size)]
        out, s = [], ts - jrem(ts - self.offset + self.slide, self.slide)  # SlidingEventTimeWindows.java:67-75
        while s > ts - self.size:
            out.append(s)
            s -= self.slide
        return out

    def _cleanup(self, start):  # WO:637-644
        c = start + self.size - 1 + self.lateness
        return c if c <= LMAX else LMAX

    def _empty(self):  # CountSumMinMax.createAccumulator: the sum starts from +0.0
        return [0, 0.0 if self.value_type == "double" else 0, None, None, 0]

    def process(self, keys, ts, vals):
        for k, t, v in zip(keys.tolist(), ts.tolist(), vals.tolist()):
            x = _f(v) if self.value_type == "double" else v
            skipped = True
            for s in self._windows(t):
                if self._cleanup(s) <= self.wm:  # isWindowLate, WO:591-593: dropped for this window (WO:381-384)
                    continue
                skipped = False
                a = self.state.setdefault((k, s), self._empty())
                a[0] += 1  # windowState.add, WO:386-387
                a[1] += x
                a[2] = x if a[2] is None or x < a[2] else a[2]
                a[3] = x if a[3] is None or x > a[3] else a[3]
                a[4] += 1  # CT:47-55: count.add(1); count >= maxCount -> clear, FIRE (the comparison is >=)
                if a[4] >= self.n:
                    a[4] = 0
                    self._rows.append(self._row(k, s, a))  # WO:395-401 emitWindowContents
                    if self.purging:  # PT: FIRE -> FIRE_AND_PURGE; WO:403-405 windowState.clear()
                        a[0:4] = self._empty()[0:4]
                # registerCleanupTimer, WO:406: the entry stays (emptied ones too) until the cleanup time
            if skipped and t + self.lateness <= self.wm:  # WO:409-419: side output or numLateRecordsDropped
                if self.side_output:
                    self._side.append((self.epoch, k, t, v))
                else:
                    self.late_dropped += 1

    def _row(self, k, s, a):
        if self.value_type == "double":
            return (self.epoch, k, s, s + self.size, a[0], _b(a[1]), _b(a[2]), _b(a[3]))
        sm = wrap32(a[1]) if self.value_type == "int" else (a[1] + (1 << 63)) % (1 << 64) - (1 << 63)
        return (self.epoch, k, s, s + self.size, a[0], sm, a[2], a[3])

    def watermark(self, wm):
        # onEventTime: CT:57-60 CONTINUE, so nothing fires; at the cleanup time clearAllState drops the accumulator
        # and the count (WO:461-463, CT:67-70): a window's last < n elements are never emitted
        for kw in [kw for kw in self.state if self._cleanup(kw[1]) <= wm]:
            del self.state[kw]
        self.wm = wm
        self.epoch += 1

    def restore(self, key, start, count, sm, mn, mx, trigger_count):
        """a snapshot row; a row of a window already present merges (AggregateFunction.merge) and the counts add
        without firing (CT:77-85 onMerge -> mergePartitionedState of the Sum ReducingState)"""
        a = self.state.setdefault((key, start), self._empty())
        if count:
            a[0] += count
            a[1] += sm
            a[2] = mn if a[2] is None or mn < a[2] else a[2]
            a[3] = mx if a[3] is None or mx > a[3] else a[3]
        a[4] += trigger_count

    def rows(self):
        return sorted(self._rows)

    def side_rows(self):
        return sorted(self._side)

    @property
    def num_state_entries(self):  # the windows with contents (the list operator's definition)
        return sum(1 for a in self.state.values() if a[0] > 0)

    @property
    def num_timers(self):  # one cleanup timer per window in flight, emptied ones included
        return sum(1 for kw in self.state if self._cleanup(kw[1]) != LMAX)
