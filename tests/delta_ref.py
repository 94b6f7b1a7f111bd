"""A plain-Python restatement of WindowOperator / EvictingWindowOperator over ListState under DeltaTrigger, element by
element: the checker of the GPU list operator's FW_TRIGGER_DELTA.  It reuses ContinuousRef (tests/continuous_ref.py) for
window assignment, lateness, the timer set, CountEvictor / TimeEvictor and cleanup, and restates what this trigger
changes.  Sources (flink-streaming-java, org/apache/flink/streaming/):
  api/windowing/triggers/DeltaTrigger.java:53-64 onElement: "last-element" null -> update, CONTINUE;
      getDelta(last, element) > threshold -> update, FIRE; else CONTINUE;  :67-75 onEventTime / onProcessingTime:
      CONTINUE (no timer is ever registered);  :78-80 clear: the state is dropped
  api/windowing/triggers/PurgingTrigger.java:45-59 FIRE -> FIRE_AND_PURGE: windowState.clear(), the trigger's state stays
  runtime/operators/windowing/EvictingWindowOperator.java:172-222 processElement (add, onElement, emitWindowContents,
      purge, registerCleanupTimer), :241-286 onEventTime, :334-366 emitWindowContents (evictBefore, the function,
      evictAfter, the survivors written back), :368-385 clearAllState (windowState, triggerContext.clear)
  api/windowing/evictors/DeltaEvictor.java:72-80: drops e with getDelta(e, last) >= threshold
  api/functions/windowing/delta/DeltaFunction.java: the built-in forms are field differences, computed in the field's
      Java arithmetic and widened to double: Long and Integer wrap at their width, Short / Byte promote to int, Double
      in double, Float in float (JLS 15.18.2, 5.6.2).
The interface is ContinuousRef's."""
import numpy as np

from tests.continuous_ref import LMAX, LMIN, ContinuousRef, _bits, _dkey, _f64, jwrap  # noqa: F401

NAN_BITS = 0x7ff8000000000000
_WIDTH = {"i64": 64, "i32": 32, "i16": 16, "i8": 8}


def _wrap(x, bits):
    return (x + (1 << (bits - 1))) % (1 << bits) - (1 << (bits - 1))


def field_delta(value_type, old, new):
    """new.field - old.field as the built-in DeltaFunction computes it; old / new are the handle's value bits"""
    if value_type == "i64":
        return float(_wrap(new - old, 64))
    if value_type in ("i32", "i16", "i8"):  # int arithmetic (Short / Byte promote): wraps at 32 bits
        return float(_wrap(new - old, 32))
    with np.errstate(invalid="ignore", over="ignore"):
        if value_type == "f32":
            return float(np.float32(_f64(new)) - np.float32(_f64(old)))
        return float(np.float64(_f64(new)) - np.float64(_f64(old)))


def canon_nan(bits):
    """Double.doubleToLongBits: every NaN is the canonical one"""
    return NAN_BITS if _f64(bits) != _f64(bits) else bits


class DeltaRef(ContinuousRef):
    def __init__(self, assigner="tumbling", size=0, slide=0, offset=0, lateness=0, threshold=0.0, purging=False,
                 evictor="none", evict_after=False, evict_arg=0, evict_threshold=0.0, side_output=False,
                 value_type="i64", greater_equal=False, update_always=False):
        assert assigner in ("tumbling", "sliding", "global")  # (a merging assigner refuses the trigger)
        assert evictor in ("none", "count", "time", "delta") and value_type in ("i64", "i32", "i16", "i8", "f64", "f32")
        super().__init__(assigner=assigner, size=size, slide=slide, offset=offset, lateness=lateness,
                         trigger="event_time", purging=purging, evictor="none", evict_after=evict_after,
                         evict_arg=evict_arg, side_output=side_output, value_type="i64")
        self.evictor, self.value_type = evictor, value_type
        self.threshold, self.evict_threshold = float(threshold), float(evict_threshold)
        self.last = {}  # (key, window) -> the value bits of "last-element"
        # mutations for the tests that show what a fixture pins (never set by a parity test)
        self.greater_equal, self.update_always = greater_equal, update_always
        # what a seeded stream exercised
        self.hits = dict(equal=0, nan=0, wrapped=0, after_purge=0, reopened=0, time_cutoff=0, first_of_push=0)
        self._emptied, self._cleaned_keys, self._push_seen = set(), set(), set()

    # ------------------------------------------------------------------ the trigger (DeltaTrigger.java:53-80)
    def _on_element_delta(self, key, w, val):
        last = self.last.get((key, w))
        if last is None:
            self.last[(key, w)] = val
            return False
        d = field_delta(self.value_type, last, val)
        if d != d:
            self.hits["nan"] += 1
        elif d == self.threshold:
            self.hits["equal"] += 1
        if self.value_type in _WIDTH and d != float(val - last):
            self.hits["wrapped"] += 1
        fire = d >= self.threshold if self.greater_equal else d > self.threshold
        if fire or self.update_always:
            self.last[(key, w)] = val
        return fire

    def _on_event_time(self, t, key, w):
        return False  # CONTINUE

    def _trigger_clear(self, key, w):
        self.last.pop((key, w), None)

    # ------------------------------------------------------------------ evictors (DeltaEvictor added)
    def _evict(self, lst):
        if self.evictor == "delta":
            if lst:
                last = lst[-1][1]
                lst[:] = [e for e in lst if not field_delta(self.value_type, e[1], last) >= self.evict_threshold]
            return
        if self.evictor == "time" and lst and lst[0][0] != LMIN:
            cutoff = jwrap(max(e[0] for e in lst) - self.evict_arg)
            self.hits["time_cutoff"] += sum(1 for e in lst if e[0] == cutoff)
        super()._evict(lst)

    # ------------------------------------------------------------------ the row's built-in reduce in every field type
    def _emit(self, key, w, sk):
        lst = self.state[sk]
        if self.evictor != "none" and not self.evict_after:
            self._evict(lst)
        seen = list(lst)
        vt = self.value_type
        if vt in ("f64", "f32"):
            with np.errstate(invalid="ignore", over="ignore"):
                s = np.float64(0.0)
                for i, e in enumerate(seen):
                    d = np.float64(_f64(e[1]))
                    s = d if i == 0 else (np.float64(np.float32(s) + np.float32(d)) if vt == "f32" else s + d)
            total = _bits(float(s))
            order = lambda b: _dkey(canon_nan(b))  # noqa: E731  Double.compare: NaN above +Infinity
            mn = canon_nan(min((e[1] for e in seen), key=order, default=0))
            mx = canon_nan(max((e[1] for e in seen), key=order, default=0))
        else:
            total = 0
            for e in seen:
                total = _wrap(total + e[1], 64)
            total = _wrap(total, _WIDTH[vt])
            mn = min((e[1] for e in seen), default=0)
            mx = max((e[1] for e in seen), default=0)
        self._rows.append((key, w[0], w[1], len(seen), total, mn, mx, seen[0][2] if seen else -1, len(self._elems),
                           self.epoch))
        self._elems.extend(seen)
        if self.evictor != "none":
            if self.evict_after:
                self._evict(lst)
            if not lst:
                del self.state[sk]

    # ------------------------------------------------------------------ processElement (EvictingWindowOperator:172-222)
    def _element(self, key, ts, val):
        o = self.ordinal
        self.ordinal += 1
        skipped = True
        for w in self._assign(ts):
            if self._window_late(w):
                continue
            sk = (key, w)
            skipped = False
            if sk not in self.state and sk in self._emptied:
                self.hits["after_purge"] += 1
                self._emptied.discard(sk)
            if sk not in self.state and sk not in self.last and key in self._cleaned_keys:
                self.hits["reopened"] += 1
            self.state.setdefault(sk, []).append((ts, val, o))
            first_of_push = sk not in self._push_seen
            self._push_seen.add(sk)
            if self._on_element_delta(key, w, val):
                self.hits["first_of_push"] += first_of_push
                self._emit(key, w, sk)
                if self.purging:
                    self.state.pop(sk, None)
                    self._emptied.add(sk)
            ct = self._cleanup_time(w)  # registerCleanupTimer: the window's only timer
            if ct != LMAX:
                self._register(ct, key, w)
        if skipped and self._event_time() and jwrap(ts + self.lateness) <= self.wm:
            if self.side_output:
                self._side.append((self.epoch, key, ts, val))
            else:
                self.late_dropped += 1

    def process(self, keys, ts, vals):
        self._push_seen = set()  # one call = one push
        super().process(keys, ts, vals)

    def _clear_all(self, key, w, sk):
        self._cleaned_keys.add(key)
        super()._clear_all(key, w, sk)


def top_speeds(cars, threshold=50.0, evictor_ms=10000, ref_kw=None, later_on_ties=False):
    """TopSpeedWindowing (TopSpeedWindowing.java:71-87) over (car, speed, distance, ts) records through DeltaRef: the
    trigger and the evictor read the distance and the timestamps, maxBy(1) picks each firing's record with the highest
    speed, the earlier one on ties (ComparableAggregator.java:73-91 with first = true)."""
    kw = dict(assigner="global", threshold=threshold, evictor="time", evict_arg=evictor_ms, value_type="f64")
    kw.update(ref_kw or {})
    ref = DeltaRef(**kw)
    for c, _, d, t in cars:
        ref.process([c], [t], np.array([d], dtype=np.float64))
    return max_by_speed(cars, ref.contents(), later_on_ties)


def max_by_speed(cars, contents, later_on_ties=False):
    """the host's maxBy(1) over every firing's contents, through the arrival ordinals"""
    out = []
    for _, el in contents:
        name = "ordinal" if "ordinal" in el.dtype.names else "ord"
        best = None
        for o in el[name].tolist():
            if best is None or cars[o][1] > cars[best][1] or (later_on_ties and cars[o][1] == cars[best][1]):
                best = o
        out.append(tuple(cars[best]))
    return out
