"""Sequential restatement of flink-table's row-time OVER ProcessFunctions, kept in the shape of the Scala
(flink-libraries/flink-table/src/main/scala/org/apache/flink/table/runtime/aggregate/):

  RowTimeBoundedRangeOver.scala:109-247   processElement / onTimer of RANGE BETWEEN t PRECEDING AND CURRENT ROW
  RowTimeBoundedRowsOver.scala:118-267    ... of ROWS BETWEEN n PRECEDING AND CURRENT ROW (precedingOffset = n + 1,
                                          plan/nodes/datastream/DataStreamOverAggregate.scala:252-275)
  RowTimeUnboundedOver.scala:103-336      ... of UNBOUNDED PRECEDING, with the ROWS and RANGE subclasses

Per key: a dict row time -> list of rows (the MapState), the accumulators with accumulate / retract, dataCount,
lastTriggeringTs (an unset ValueState[Long] reads as 0).  Plain Python, independent of the product code.
Idle-state retention (the processing-time clean-up timers) is not restated: the default StreamQueryConfig has none.
"""
import math

LMIN, LMAX = -(1 << 63), (1 << 63) - 1
_BITS = {"long": 64, "int": 32, "short": 16, "byte": 8}


def _wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _tdiv(s, c):
    q = abs(s) // c
    return -q if s < 0 else q


class _Agg:
    """One built-in aggregate with retraction (functions/aggfunctions/*WithRetractAggFunction.scala, CountAggFunction,
    AvgAggFunction): getValue is None (SQL NULL) while no non-null value is accumulated, except for the counts."""

    def __init__(self, fn, typ):
        self.fn, self.typ = fn, typ
        self.count = 0
        self.sum = 0.0 if typ in ("double", "float") else 0
        self.values = []

    def accumulate(self, v):
        if self.fn == "count_star":
            self.count += 1
            return
        if v is None:
            return
        self.count += 1
        if self.fn in ("min", "max"):
            self.values.append(v)
        elif self.fn in ("sum", "avg"):
            self.sum = self.sum + v
            if self.typ in _BITS:
                # SUM wraps to the column's width; an Integral AVG sums in a Long; the Long AVG's sum does not wrap
                bits = _BITS[self.typ] if self.fn == "sum" else (64 if self.typ != "long" else None)
                if bits:
                    self.sum = _wrap(self.sum, bits)

    def retract(self, v):
        if self.fn == "count_star":
            self.count -= 1
            return
        if v is None:
            return
        self.count -= 1
        if self.fn in ("min", "max"):
            self.values.remove(v)
        elif self.fn in ("sum", "avg"):
            self.sum = self.sum - v
            if self.typ in _BITS:
                bits = _BITS[self.typ] if self.fn == "sum" else (64 if self.typ != "long" else None)
                if bits:
                    self.sum = _wrap(self.sum, bits)

    def value(self):
        if self.fn in ("count_star", "count"):
            return self.count
        if self.count == 0:
            return None
        if self.fn == "sum":
            return self.sum
        if self.fn == "min":
            return min(self.values)
        if self.fn == "max":
            return max(self.values)
        if self.typ in ("double", "float"):
            return self.sum / self.count
        q = _tdiv(self.sum, self.count)
        return q if self.typ == "long" else _wrap(q, _BITS[self.typ])


class _Key:
    def __init__(self):
        self.data = {}            # MapState[Long, JList[Row]]; a row is (ordinal, rowtime, [values])
        self.acc = None           # accumulatorState
        self.data_count = 0       # dataCountState (bounded ROWS)
        self.last_ts = 0          # lastTriggeringTsState.value of an unset state unboxes to 0L


class OverRef:
    def __init__(self, kind, preceding, column_types, aggregates):
        assert kind in ("bounded_rows", "bounded_range", "unbounded_rows", "unbounded_range")
        self.kind = kind
        self.bounded = kind.startswith("bounded")
        # DataStreamOverAggregate.scala:252-275: ROWS frames get precedingOffset = N + 1
        self.preceding_offset = preceding + 1 if kind == "bounded_rows" else preceding
        self.column_types = list(column_types)
        self.aggregates = [(f, int(c)) for f, c in aggregates]
        self.keys = {}
        self.wm = LMIN
        self.ordinal = 0
        self.kept = self.late = 0

    # ---- function.createAccumulators / accumulate / retract / setAggregationResults
    def _create(self):
        return [_Agg(f, self.column_types[c] if f != "count_star" else "long") for f, c in self.aggregates]

    def _accumulate(self, acc, row):
        for a, (f, c) in zip(acc, self.aggregates):
            a.accumulate(None if f == "count_star" else row[2][c])

    def _retract(self, acc, row):
        for a, (f, c) in zip(acc, self.aggregates):
            a.retract(None if f == "count_star" else row[2][c])

    @staticmethod
    def _results(acc):
        return [a.value() for a in acc]

    # ---- processElement
    def process(self, keys, rowtimes, columns, nulls=None):
        for i in range(len(keys)):
            vals = [None if nulls is not None and (int(nulls[i]) >> j) & 1 else
                    (float(col[i]) if self.column_types[j] in ("double", "float") else int(col[i]))
                    for j, col in enumerate(columns)]
            self.process_element(int(keys[i]), int(rowtimes[i]), vals)

    def process_element(self, key, ts, vals):
        row = (self.ordinal, ts, vals)
        self.ordinal += 1
        st = self.keys.get(key)
        if self.bounded:
            last = st.last_ts if st is not None else 0
            keep = ts > last                      # triggeringTs > lastTriggeringTs
        else:
            keep = ts > self.wm                   # timestamp > curWatermark
        if not keep:
            self.late += 1
            return
        self.kept += 1
        if st is None:
            st = self.keys[key] = _Key()
        st.data.setdefault(ts, []).append(row)

    # ---- the timer service: every registered row time <= wm, per key in ascending order
    def watermark(self, wm):
        assert wm >= self.wm
        self.wm = wm
        out = []
        for key, st in self.keys.items():
            if self.bounded:
                for t in sorted(t for t in st.data if st.last_ts < t <= wm):
                    (self._on_timer_range if self.kind == "bounded_range" else self._on_timer_rows)(key, st, t, out)
            else:
                self._on_timer_unbounded(key, st, out)
        return out

    def _emit(self, out, key, row, acc):
        out.append((key, row[1], row[0], self._results(acc)))

    def _on_timer_range(self, key, st, timestamp, out):   # RowTimeBoundedRangeOver.scala:140-247
        inputs = st.data.get(timestamp)
        if inputs is not None:
            if st.acc is None:
                st.acc = self._create()
            retract_ts = []
            for data_ts in list(st.data):
                offset = timestamp - data_ts
                if offset > self.preceding_offset:
                    for r in st.data[data_ts]:
                        self._retract(st.acc, r)
                    retract_ts.append(data_ts)
            for r in inputs:
                self._accumulate(st.acc, r)
            for r in inputs:
                self._emit(out, key, r, st.acc)
            for t in retract_ts:
                del st.data[t]
        st.last_ts = timestamp

    def _on_timer_rows(self, key, st, timestamp, out):    # RowTimeBoundedRowsOver.scala:149-267
        inputs = st.data.get(timestamp)
        if inputs is not None:
            retract_list, retract_ts, retract_cnt = None, LMAX, 0
            for r in inputs:
                if st.acc is None:
                    st.acc = self._create()
                retract_row = None
                if st.data_count >= self.preceding_offset:
                    if retract_list is None:
                        retract_ts = min(st.data)
                        retract_list = st.data[retract_ts]
                    retract_row = retract_list[retract_cnt]
                    retract_cnt += 1
                    if len(retract_list) == retract_cnt:
                        del st.data[retract_ts]
                        retract_list, retract_cnt = None, 0
                else:
                    st.data_count += 1
                if retract_row is not None:
                    self._retract(st.acc, retract_row)
                self._accumulate(st.acc, r)
                self._emit(out, key, r, st.acc)
            if retract_ts in st.data and retract_cnt > 0:
                del retract_list[:retract_cnt]
        st.last_ts = timestamp

    def _on_timer_unbounded(self, key, st, out):          # RowTimeUnboundedOver.scala:140-211, :267-335
        due = sorted(t for t in st.data if t <= self.wm)
        if not due:
            return
        if st.acc is None:
            st.acc = self._create()
        for t in due:
            rows = st.data.pop(t)
            if self.kind == "unbounded_rows":
                for r in rows:
                    self._accumulate(st.acc, r)
                    self._emit(out, key, r, st.acc)
            else:
                for r in rows:
                    self._accumulate(st.acc, r)
                for r in rows:
                    self._emit(out, key, r, st.acc)

    # ---- what the handle's statistics count
    def stats(self):
        pending = retained = 0
        for st in self.keys.values():
            for t, rows in st.data.items():
                if not self.bounded or t > st.last_ts:
                    pending += len(rows)
                else:
                    retained += len(rows)
        return {"rows_kept": self.kept, "late_rows_dropped": self.late, "keys": len(self.keys),
                "retained_rows": retained, "pending_rows": pending}


def close(a, b, rtol):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) or isinstance(b, float):
        return math.isclose(a, b, rel_tol=rtol, abs_tol=0.0) or a == b
    return a == b
