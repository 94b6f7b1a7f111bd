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
import struct

LMIN, LMAX = -(1 << 63), (1 << 63) - 1
_BITS = {"long": 64, "int": 32, "short": 16, "byte": 8}


def _wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _tdiv(s, c):
    q = abs(s) // c
    return -q if s < 0 else q


NAN_BITS = 0x7FF8000000000000


def double_bits(v):
    """Double.doubleToLongBits: the signed 64 bits, every NaN the canonical one"""
    return NAN_BITS if v != v else struct.unpack("<q", struct.pack("<d", v))[0]


def _compare(a, b):
    """ord.compare: Ordering.Double.compare is java.lang.Double.compare (Scala 2.11.12) -- numeric order, then the
    doubleToLongBits, so -0.0 < 0.0 and NaN == NaN is above +Inf; Ordering.Long etc. are the plain order"""
    if a < b:
        return -1
    if a > b:
        return 1
    if isinstance(a, float) or isinstance(b, float):
        x, y = double_bits(a), double_bits(b)
        return (x > y) - (x < y)
    return 0


class _Agg:
    """One built-in aggregate (functions/aggfunctions/): getValue is None (SQL NULL) while no non-null value is
    accumulated, except for the counts.

    Bounded kinds get the retracting functions, unbounded kinds the plain ones (AggregateUtil.scala:230-236
    `needRetract = true` in createBoundedOverProcessFunction, :86-91 `needRetraction = false` in
    createUnboundedOverProcessFunction; the choice itself at :1158-1347).

    MIN / MAX with retraction (MinAggFunctionWithRetract.scala:50-100, MaxAggFunctionWithRetract.scala:50-100), line
    for line: a HashMap value -> count whose keys are boxed values (Double.equals / hashCode: by doubleToLongBits,
    NaN canonical, -0.0 != 0.0), the current extreme f0 chosen by ord.compare, `v == acc.f0` on retraction (boxed
    `==`: numeric equality, false for NaN, true for -0.0 against 0.0), f0 back to the initial value when the map
    empties.  So a MAX whose NaN leaves while other values remain keeps the NaN: it is not rescanned.
    MIN / MAX without retraction (MinAggFunction.scala / MaxAggFunction.scala:49-57): f0 and a flag, ord.compare.

    SUM / AVG: plain sequential `+` and `-` from +0.0 / 0 (SumWithRetractAggFunction.scala:43-60, SumAggFunction.scala
    :39-53, AvgAggFunction.scala:214-242), so a sum of only -0.0 is +0.0, a retracted infinity leaves Inf - Inf = NaN
    and a non-finite sum never becomes finite again."""

    def __init__(self, fn, typ, retract=True):
        self.fn, self.typ, self.retracting = fn, typ, retract
        self.count = 0
        self.floating = typ in ("double", "float")
        self.sum = 0.0 if self.floating else 0
        self.f0 = self.init = 0.0 if self.floating else 0   # getInitValue
        self.map = {}                                       # key -> [the boxed value, its count]
        self.f1 = False
        self.sign = -1 if fn == "max" else 1                # MAX: ord.compare(f0, v) < 0; MIN: > 0

    def _key(self, v):
        return double_bits(v) if self.floating else v

    def accumulate(self, v):
        if self.fn == "count_star":
            self.count += 1
            return
        if v is None:
            return
        self.count += 1
        if self.fn in ("min", "max"):
            if not self.retracting:
                if not self.f1 or _compare(self.f0, v) * self.sign > 0:
                    self.f0 = v
                    self.f1 = True
                return
            if len(self.map) == 0 or _compare(self.f0, v) * self.sign > 0:
                self.f0 = v
            k = self._key(v)
            if k not in self.map:
                self.map[k] = [v, 1]
            else:
                self.map[k][1] += 1
        elif self.fn in ("sum", "avg"):
            self.sum = self.sum + v
            if self.typ in _BITS:
                # SUM wraps to the column's width; an Integral AVG sums in a Long; the Long AVG's sum does not wrap
                bits = _BITS[self.typ] if self.fn == "sum" else (64 if self.typ != "long" else None)
                if bits:
                    self.sum = _wrap(self.sum, bits)

    def retract(self, v):
        assert self.retracting
        if self.fn == "count_star":
            self.count -= 1
            return
        if v is None:
            return
        self.count -= 1
        if self.fn in ("min", "max"):
            k = self._key(v)
            count = self.map[k][1] - 1
            if count == 0:
                del self.map[k]
                if len(self.map) == 0:
                    self.f0 = self.init
                    return
                if v == self.f0:                            # numeric: never true for NaN
                    it = iter(self.map.values())
                    self.f0 = next(it)[0]
                    for key, _ in it:
                        if _compare(self.f0, key) * self.sign > 0:
                            self.f0 = key
            else:
                self.map[k][1] = count
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
        if self.fn in ("min", "max"):
            return self.f0
        if self.floating:
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
        return [_Agg(f, self.column_types[c] if f != "count_star" else "long", retract=self.bounded)
                for f, c in self.aggregates]

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
