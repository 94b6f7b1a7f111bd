// fw_range.h — host arithmetic on timestamps at the ends of the long range (DESIGN.md "Event-time arithmetic"): the
// refusals of FW_ERR_TIME_RANGE as the host decides them for host columns (classify's CLS_RANGE restated), the list
// operator's runaway test (host and device), and the compact records' base.  Plain wrapping 64-bit and 128-bit
// arithmetic, no HIP: oracle/sanitize_main.cpp runs every function here under ASan + UBSan at both ends of the range.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FW_RANGE_HD __host__ __device__
#else
#define FW_RANGE_HD
#endif

FW_RANGE_HD inline int64_t fw_wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
FW_RANGE_HD inline int64_t fw_wsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }

// what classify needs to know of a sliding operator: wpr = ceil(size / slide) + 1
struct fw_range_cfg {
  int64_t size, slide, offset;
  int32_t wpr;
  bool panes, tdigest;
};
// is ts refused by the sliding operator c (ts != Long.MIN_VALUE)?
//  * kept as panes: the newest window's end, or ts - offset + slide, wraps past Long.MAX_VALUE, or ts lies within
//    size + 2 slide of Long.MIN_VALUE;
//  * kept as windows: the runaway set (the walk has not ended after wpr windows), and for a t-digest a record with
//    several windows of which the newest one's end wraps.
FW_RANGE_HD inline bool fw_time_range_record(const fw_range_cfg& c, int64_t ts) {
  const int64_t u = fw_wsub(ts, c.offset), t = fw_wadd(u, c.slide);
  const int64_t last = fw_wsub(ts, t % c.slide), lo = fw_wsub(ts, c.size);
  const int64_t newest_end = fw_wadd(last, c.size);
  if (c.panes) {
    const int64_t b = fw_wsub(lo, c.slide), d = fw_wsub(b, c.slide);
    return newest_end < last || t < u || lo > ts || b > lo || d > b;
  }
  int k = 0;
  int64_t s = last;
  for (; s > lo && k < c.wpr; s = fw_wsub(s, c.slide)) k++;
  if (k <= 1) return false;
  if (newest_end < last) return c.tdigest;
  return k == c.wpr && s > lo;
}
// only a timestamp at or below *lo or at or above *hi can be refused: within size + 2 slide of an end
inline void fw_range_guards(int64_t size, int64_t slide, int64_t* lo, int64_t* hi) {
  __int128 g = (__int128)size + 2 * (__int128)slide;
  if (g > (__int128)INT64_MAX) g = INT64_MAX;
  *lo = (int64_t)((__int128)INT64_MIN + g);
  *hi = (int64_t)((__int128)INT64_MAX - g);
}
// the runaway set of the sliding assigner (size, slide, offset), wcap = ceil(size / slide) + 1: a timestamp just above
// Long.MIN_VALUE + size, where ts - size does not wrap but the walk down from the newest start does, past
// Long.MIN_VALUE to the top of the range; the reference's own loop then runs for about 2^64 / slide steps
FW_RANGE_HD inline bool fw_sliding_runaway(int64_t size, int64_t slide, int64_t offset, int64_t wcap, int64_t ts) {
  // (the walk covers at most size + 2 slide <= 3 size from the newest start, which lies below ts + slide)
  if (size < (int64_t(1) << 61) && (uint64_t)ts - (uint64_t)INT64_MIN >= 4 * (uint64_t)size) return false;
  const int64_t lo = fw_wsub(ts, size);
  int64_t s = fw_wsub(ts, fw_wadd(fw_wsub(ts, offset), slide) % slide);
  for (int64_t k = 0; k < wcap; k++) {
    if (!(s > lo)) return false;
    s = fw_wsub(s, slide);
  }
  return s > lo;
}
// ContinuousEventTimeTrigger.onElement's first fire time of a window, from the element that finds the trigger's
// "fire-time" state null: start = timestamp - (timestamp % interval), nextFireTimestamp = start + interval
// (ContinuousEventTimeTrigger.java:64-65; Java's truncating %, wrapping longs; iv > 0)
FW_RANGE_HD inline int64_t fw_first_fire(int64_t ts, int64_t iv) { return fw_wadd(fw_wsub(ts, ts % iv), iv); }
// The aggregating operator under ContinuousEventTimeTrigger refuses a record with ts > Long.MAX_VALUE - interval: its
// first fire time, or the timer the trigger registers after that one (fire + interval), wraps past Long.MAX_VALUE,
// and the chain of early firings would go on from the bottom of the long range (DESIGN.md "Event-time arithmetic",
// excluded class (2))
FW_RANGE_HD inline bool fw_first_fire_wraps(int64_t ts, int64_t iv) { return ts > INT64_MAX - iv; }

// compact records: window deltas count from 2^(log_s - 1) windows (or panes) before the watermark's, so a batch's
// windows on both sides of the watermark fit; false: no base (it leaves the long range near Long.MIN_VALUE)
inline bool fw_compact_base(int64_t wm, int64_t offset, int64_t slide, int log_s, int64_t* base) {
  const __int128 u = slide, w = wm, off = offset;
  __int128 q = (w - off) / u;
  if ((w - off) % u < 0) q -= 1;  // floor
  const __int128 b = q * u + off - ((__int128)1 << (log_s - 1)) * u;
  if (b < (__int128)INT64_MIN || b > (__int128)INT64_MAX) return false;
  *base = (int64_t)b;
  return true;
}
