// fw_cont.h — ContinuousEventTimeTrigger on the aggregating operator: the trigger state an entry carries and what one
// watermark does to it, in closed form (no loop over the timers).  Plain wrapping 64-bit arithmetic, host and device,
// no HIP: the firing kernels (fw_device.hip, k_cf_count / k_cf_fire) and the stand-alone checks use the same text.
//
// ContinuousEventTimeTrigger.java:53-92 under WindowOperator.onEventTime (WindowOperator.java:424-469).  A window's
// trigger state is `fire` (the "fire-time" ReducingState, Min; null allowed) and at most two registered timers:
// maxTimestamp M and fire.  One watermark runs the window's timers t <= L = min(wm, cleanupTime) in ascending time:
//   contents == null: the timer is consumed, the trigger is not asked (a fire timer is then not re-armed);
//   t == M:           FIRE, fire untouched (with fire == M that is one timer, and early firing has stopped for good);
//   t == fire != M:   FIRE, fire = t + interval, a timer there.
// No element arrives between two timers of one advance, so without PurgingTrigger every firing emits the same row and
// under it only the first one emits (the later timers run over null contents).
//
// In the entry: meta bit 0 = M's timer (FW_TIMER), bit 1 = the timer at `fire` is registered, bit 2 = fire is not
// null, bits 3..63 = fire - window start, signed (fw_create bounds size + lateness + 2 interval by 2^60, so it fits;
// negative for a pre-epoch element whose window starts above it, TimeWindow.getWindowStartWithOffset's truncating %).
#pragma once
#include <cstdint>
#include "fw_range.h"

enum : uint32_t { FW_CF_MTIMER = 1, FW_CF_REG = 2, FW_CF_SET = 4 };
enum { FW_CF_SHIFT = 3 };
#define FW_CF_MAX_SPAN ((int64_t)1 << 60)  // size + allowed lateness + 2 * interval, at most
#define FW_CF_MAX_FIRINGS ((uint64_t)1 << 20)  // of one window in one advance

FW_RANGE_HD inline uint32_t fw_cf_flags(int64_t meta) { return (uint32_t)meta & 7u; }
FW_RANGE_HD inline int64_t fw_cf_fire(int64_t meta, int64_t start) {
  return (int64_t)((uint64_t)start + (uint64_t)(meta >> FW_CF_SHIFT));  // (arithmetic shift: the offset's sign)
}
// false: fire - start does not fit (a window that wraps around the long range)
FW_RANGE_HD inline bool fw_cf_pack(int64_t start, int64_t fire, uint32_t fl, int64_t* meta) {
  const int64_t d = (int64_t)((uint64_t)fire - (uint64_t)start);
  *meta = (int64_t)(((uint64_t)d << FW_CF_SHIFT) | (fl & 7u));
  return d >= -FW_CF_MAX_SPAN && d < FW_CF_MAX_SPAN;
}

// rows the window fires at watermark wm: the fire times fire + j * interval <= L up to and with M if they meet it,
// plus M if it is registered and not met; one at the most under PurgingTrigger, none over null contents
FW_RANGE_HD inline uint64_t fw_cf_count(int64_t M, int64_t C, int64_t fire, uint32_t fl, int64_t iv, bool purging,
                                        bool contents, int64_t wm) {
  if (!contents) return 0;
  const int64_t L = wm < C ? wm : C;
  uint64_t k = 0;
  bool met = false;
  if ((fl & FW_CF_REG) && fire <= L) {
    k = ((uint64_t)L - (uint64_t)fire) / (uint64_t)iv + 1;
    if (M >= fire && M <= L && ((uint64_t)M - (uint64_t)fire) % (uint64_t)iv == 0) {
      k = ((uint64_t)M - (uint64_t)fire) / (uint64_t)iv + 1;
      met = true;
    }
  }
  if ((fl & FW_CF_MTIMER) && M <= L && !met) k++;
  return purging && k > 1 ? 1 : k;
}

// the trigger state after those timers; *cleared = PurgingTrigger emptied the contents
FW_RANGE_HD inline void fw_cf_advance(int64_t M, int64_t C, int64_t iv, bool purging, bool contents, int64_t wm,
                                      int64_t* fire, uint32_t* fl, bool* cleared) {
  const int64_t L = wm < C ? wm : C;
  const bool fdue = (*fl & FW_CF_REG) && *fire <= L, mdue = (*fl & FW_CF_MTIMER) && M <= L;
  *cleared = false;
  if (!contents) {  // consumed without asking the trigger
    if (mdue) *fl &= ~FW_CF_MTIMER;
    if (fdue) *fl &= ~FW_CF_REG;
    return;
  }
  if (!purging) {
    if (fdue) {
      const int64_t f = *fire;
      if (M >= f && M <= L && ((uint64_t)M - (uint64_t)f) % (uint64_t)iv == 0) {
        *fire = M;  // the chain met maxTimestamp: stuck there
        *fl &= ~FW_CF_REG;
      } else {
        const uint64_t n = ((uint64_t)L - (uint64_t)f) / (uint64_t)iv + 1;
        const int64_t last = (int64_t)((uint64_t)f + (n - 1) * (uint64_t)iv), nx = fw_wadd(last, iv);
        if (nx > last) {
          *fire = nx;
        } else {  // past Long.MAX_VALUE: nothing more is registered
          *fire = last;
          *fl &= ~FW_CF_REG;
        }
      }
    }
    if (mdue) *fl &= ~FW_CF_MTIMER;
    return;
  }
  // PurgingTrigger: the earliest due timer fires and purges, the later ones run over null contents
  if (fdue && (!mdue || *fire < M)) {
    const int64_t t = *fire;
    if (t == M) {
      *fl &= ~FW_CF_REG;
    } else {
      const int64_t nx = fw_wadd(t, iv);
      if (nx > t) *fire = nx;
      if (!(nx > t) || nx <= L) *fl &= ~FW_CF_REG;  // (re-armed at or below L: consumed over null contents)
    }
    if (mdue) *fl &= ~FW_CF_MTIMER;
    *cleared = true;
  } else if (mdue) {
    *fl &= ~FW_CF_MTIMER;
    if (fdue) *fl &= ~FW_CF_REG;  // (fire == M is the same timer; a later one runs over null contents)
    *cleared = true;
  }
}

// the earliest pending timer of the entry: M, fire (each if registered) and the cleanup time
FW_RANGE_HD inline int64_t fw_cf_next(int64_t M, int64_t C, int64_t fire, uint32_t fl) {
  int64_t d = C;
  if ((fl & FW_CF_MTIMER) && M < d) d = M;
  if ((fl & FW_CF_REG) && fire < d) d = fire;
  return d;
}
// its event-time timers as HeapInternalTimerService's set counts them: coinciding times once
FW_RANGE_HD inline int fw_cf_timers(int64_t M, int64_t C, int64_t fire, uint32_t fl, bool has_cleanup) {
  const bool m = (fl & FW_CF_MTIMER) != 0, f = (fl & FW_CF_REG) != 0;
  int n = 0;
  if (m) n++;
  if (f && !(m && fire == M)) n++;
  if (has_cleanup && !(m && C == M) && !(f && C == fire)) n++;
  return n;
}
