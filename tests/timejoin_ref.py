"""A sequential restatement of the Table API time-windowed join on row time, one row at a time: flink-table's
runtime/join/TimeBoundedStreamJoin.scala:55-494 with RowTimeBoundedStreamJoin.scala:30-85 (operator time = max(current
watermark, 0) for both sides, event-time clean-up timers) inside runtime/operators/
KeyedCoProcessOperatorWithWatermarkDelay.scala:27-56 (the forwarded watermark is held back by getMaxOutputDelay), with a
join function that accepts every pair.  The two expiration times are fields of the operator instance (not keyed, not
checkpointed); timers are explicit: (key, time) pairs in a set, fired in time order by watermark().

Output rows are tuples (key, left_ord, right_ord, left_rowtime, right_rowtime, left_val, right_val, cause_ord,
timer_ts): ordinals count arrivals over both sides, -1 marks the null-padded side (its rowtime and val are 0);
cause_ord is the row whose processElement emitted the row (-1: a timer) and timer_ts the timer's time (-1 otherwise).
Within one call the order is the restatement's own; the reference's is hash-map iteration order, so rows are compared
as sorted multisets per call.
"""
LMAX = (1 << 63) - 1
LMIN = -(1 << 63)
INNER, LEFT, RIGHT, FULL = 0, 1, 2, 3
JOIN_TYPES = {"inner": INNER, "left": LEFT, "right": RIGHT, "full": FULL}
COUNTERS = ("rows_in", "cached_rows", "rows_not_cached", "pairs", "padded_at_arrival", "padded_at_scan",
            "padded_at_timer", "pairs_with_expired_rows", "gate_skips", "timers_set")


def _wrap(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


class _Key:
    __slots__ = ("cache", "has_map", "timer")

    def __init__(self):
        self.cache = ({}, {})         # per side: row time -> [[ord, val, emitted]], MapState[Long, List[(Row, Boolean)]]
        self.has_map = [False, False]  # the heap MapState exists (an eagerly emptied one does, until clear())
        self.timer = [0, 0]            # indexed by the cache it cleans: [rightTimerState, leftTimerState]


class TimeBoundedJoinRef:
    def __init__(self, join_type, lower, upper, allowed_lateness=0):
        self.type = JOIN_TYPES[join_type] if isinstance(join_type, str) else join_type
        if allowed_lateness < 0:
            raise ValueError("The allowed lateness must be non-negative.")
        if lower > upper:
            raise ValueError("negative window size")
        self.rel = (-lower, upper)  # leftRelativeSize, rightRelativeSize
        self.M = (self.rel[0] + self.rel[1]) // 2  # minCleanUpInterval; Java division of a sum that is never negative
        self.L = allowed_lateness
        self.X = [0, 0]  # leftExpirationTime, rightExpirationTime
        self.wm = LMIN
        self.keys = {}
        self.timers = set()  # (time, key): the internal timer service's event-time timers
        self.next_ord = 0
        for c in COUNTERS:
            setattr(self, c, 0)

    # ---- harness views
    def num_keyed_state_entries(self):
        return sum(sum(k.has_map) + sum(1 for t in k.timer if t != 0) for k in self.keys.values())

    def num_event_time_timers(self):
        return len(self.timers)

    def stats(self):
        d = {c: getattr(self, c) for c in COUNTERS}
        d["store_rows"] = sum(len(rows) for k in self.keys.values() for c in k.cache for rows in c.values())
        d["active_timers"] = sum(1 for k in self.keys.values() for t in k.timer if t != 0)
        d["current_watermark"] = self.wm
        return d

    def _pads(self, side):
        return self.type == FULL or self.type == (LEFT if side == 0 else RIGHT)

    def _T(self):
        return self.wm if self.wm > 0 else 0

    def _exp(self, c):  # calExpirationTime for cache c
        T = self._T()
        return T - self.rel[c] - self.L - 1 if T < LMAX else LMAX

    @staticmethod
    def _padded(key, side, row, t, cause, timer_ts):
        o, v = row[0], row[1]
        return (key, o, -1, t, 0, v, 0, cause, timer_ts) if side == 0 else (key, -1, o, 0, t, 0, v, cause, timer_ts)

    # ---- processElement1 (side 0) / processElement2 (side 1)
    def process(self, side, key, t, val=0):
        out = []
        s, o = side, 1 - side
        ord_ = self.next_ord
        self.next_ord += 1
        self.rows_in += 1
        T = self._T()
        lower_q, upper_q = t - self.rel[o], t + self.rel[s]
        st = self.keys.get(key)
        emitted = False
        if self.X[o] < upper_q:
            self.X[o] = self._exp(o)
            other = st.cache[o] if st is not None else {}
            for rt in list(other.keys()):
                rows = other[rt]
                if lower_q <= rt <= upper_q:
                    for row in rows:
                        out.append((key, ord_, row[0], t, rt, val, row[1], ord_, -1) if s == 0 else
                                   (key, row[0], ord_, rt, t, row[1], val, ord_, -1))
                        self.pairs += 1
                        if rt <= self.X[o]:
                            self.pairs_with_expired_rows += 1
                        emitted = True
                        if self._pads(o):
                            row[2] = True
                if rt <= self.X[o]:
                    if self._pads(o):
                        for row in rows:
                            if not row[2]:
                                out.append(self._padded(key, o, row, rt, ord_, -1))
                                self.padded_at_scan += 1
                    del other[rt]  # eager remove
        else:
            self.gate_skips += 1
        if T < upper_q:
            if st is None:
                st = self.keys[key] = _Key()
            st.cache[s].setdefault(t, []).append([ord_, val, emitted])
            st.has_map[s] = True
            self.cached_rows += 1
            if st.timer[s] == 0:
                self._register(key, st, s, t)
        else:
            self.rows_not_cached += 1
            if self._pads(s) and not emitted:
                out.append(self._padded(key, s, [ord_, val], t, ord_, -1))
                self.padded_at_arrival += 1
        return out

    def _register(self, key, st, c, row_time):  # registerCleanUpTimer for the timer that cleans cache c
        when = row_time + self.rel[c] + self.M + self.L + 1
        self.timers.add((when, key))
        st.timer[c] = when
        self.timers_set += 1

    def push(self, sides, keys, rowtimes, vals=None):
        out = []
        for i in range(len(keys)):
            out += self.process(int(sides[i]), int(keys[i]), int(rowtimes[i]), int(vals[i]) if vals is not None else 0)
        return out

    # ---- processWatermark: the timer service advances, then the delayed watermark is forwarded
    def watermark(self, wm):
        assert wm >= self.wm
        self.wm = wm
        out = []
        while self.timers:
            when, key = min(self.timers)
            if when > wm:
                break
            self.timers.discard((when, key))
            self._on_timer(when, key, out)
        return out, _wrap(wm - (max(self.rel) + self.L))

    def _on_timer(self, when, key, out):
        st = self.keys.get(key)
        if st is None:
            return
        for c in (1, 0):  # leftTimerState (cleans the right cache) first
            if st.timer[c] == when:
                self.X[c] = self._exp(c)
                earliest = -1
                cache = st.cache[c]
                for rt in list(cache.keys()):
                    if rt <= self.X[c]:
                        if self._pads(c):
                            for row in cache[rt]:
                                if not row[2]:
                                    out.append(self._padded(key, c, row, rt, -1, when))
                                    self.padded_at_timer += 1
                        del cache[rt]
                    elif rt < earliest or earliest < 0:
                        earliest = rt
                if earliest > 0:
                    self._register(key, st, c, earliest)
                else:
                    st.timer[c] = 0
                    cache.clear()
                    st.has_map[c] = False
        if st.timer == [0, 0] and not any(st.has_map):
            del self.keys[key]

    # ---- keyed state, in the shape of TimeBoundedJoin.snapshot: of the keys that `pick` accepts
    def snapshot(self, pick=lambda key: True):
        st = {f: [] for f in ("key", "left_timer", "right_timer", "n_rows", "side", "rowtime", "ordinal", "val",
                              "emitted")}
        for key in sorted(self.keys):
            k = self.keys[key]
            if not pick(key) or k.timer == [0, 0]:
                continue
            n = 0
            for c in (0, 1):
                for rt in sorted(k.cache[c]):
                    for row in k.cache[c][rt]:
                        st["side"].append(c)
                        st["rowtime"].append(rt)
                        st["ordinal"].append(row[0])
                        st["val"].append(row[1])
                        st["emitted"].append(1 if row[2] else 0)
                        n += 1
            st["key"].append(key)
            st["left_timer"].append(k.timer[1])
            st["right_timer"].append(k.timer[0])
            st["n_rows"].append(n)
        return st

    def restore(self, state):
        r = 0
        for i, key in enumerate(state["key"]):
            key = int(key)
            assert key not in self.keys
            k = self.keys[key] = _Key()
            k.timer = [int(state["right_timer"][i]), int(state["left_timer"][i])]
            for t in k.timer:
                if t != 0:
                    self.timers.add((t, key))
            rows = []
            for _ in range(int(state["n_rows"][i])):
                rows.append((int(state["side"][r]), int(state["rowtime"][r]), int(state["ordinal"][r]),
                             int(state["val"][r]), bool(state["emitted"][r])))
                r += 1
            for c, rt, o, v, e in sorted(rows, key=lambda x: x[2]):
                k.cache[c].setdefault(rt, []).append([o, v, e])
                k.has_map[c] = True
                self.next_ord = max(self.next_ord, o + 1)
