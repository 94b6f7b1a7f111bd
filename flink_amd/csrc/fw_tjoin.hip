// fw_tjoin.hip — Table API time-windowed (interval) join on row time (flink_window.h "fw_tjoin_").
//
// flink-table's RowTimeBoundedStreamJoin keeps two per-key row caches (MapState: row time -> rows) and two per-key
// clean-up timers, and scans a key's whole other cache for every arriving row.  Here the two caches are one row store
// in HBM, sorted by (group = key slot * 2 + side, row time, arrival ordinal), and a push of tagged rows is evaluated
// at once:
//   push:      check the rows, find the first row of each side that passes the operator-wide gate (a min over
//              ordinals) -> claim key slots, classify every row (cached / scans), first scanner and first cached row
//              per group (atomic mins) -> radix sort the batch by (group, row time, ordinal) -> per scanning row its
//              partner ranges by binary search: in the store (the part <= the expiration time only for the group's
//              first scanner) and among the batch's cached rows -> exclusive scan of the candidate counts -> a
//              load-balanced pass over the candidate index space that counts the pairs (a batch candidate is a pair
//              iff the partner arrived earlier) and marks the joined flags in scratch -> padding flags -> ONE read of
//              the counts by the host: refusals and the capacity check, nothing changed so far -> the same
//              load-balanced pass writes the pairs -> padded rows -> the removed rows leave and the cached batch rows
//              enter the store in one merge of two sorted runs -> timers armed by the first cached row.
//   watermark: nothing while it is below the earliest timer.  Otherwise: the due (key, side) timers -> per due run the
//              first remaining row (new timer, or the whole run is cleared when that row's time is 0) -> expired rows
//              leave, the unjoined ones padded with the timer's time -> compaction -> the earliest timer again.
// No thread walks a key's cache or a key's pairs: one key may hold every row.
#include <numeric>

#include "fw_table.h"

namespace {

constexpr int TJ_THREADS = 256, TJ_ITEMS = 4;
constexpr int TJ_CHUNK = TJ_THREADS * TJ_ITEMS;  // candidates a workgroup of the pair pass takes per step
constexpr int TJ_GRID = 1024;                    // workgroups of the pair pass: each a contiguous span of candidates
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int64_t TJ_TS_END = int64_t(1) << 62;  // row times are in [0, 2^62)
// An operator time above every bound a row can have (2^62 + 2^60) behaves like this one, and keeps T - rel - L - 1
// inside the long range
constexpr int64_t TJ_T_CLAMP = int64_t(7) << 60;

struct TCfg {
  int32_t type, key_kind, max_par, kg0, nkg, pad;
  int64_t rel[2];  // leftRelativeSize = -lower, rightRelativeSize = upper
  int64_t M, L;    // minCleanUpInterval, allowedLateness
};
// does the join type null-pad an unjoined row of `side`
__host__ __device__ inline bool tj_pads(int type, int side) {
  return type == FW_TJOIN_FULL || (side == 0 ? type == FW_TJOIN_LEFT : type == FW_TJOIN_RIGHT);
}
// what one call sees of the operator's time: the (clamped) operator time, the expiration time a scan or timer of
// cache `c` would set, and the two expiration fields as they are
struct TEpoch {
  int64_t T, E[2], X[2];
};

struct TCtr {
  // of one push (k_tj_reset)
  unsigned long long bad_time, bad_kg, bad_side, n_cached, n_scan, n_pad_arr, n_pad_scan, n_rm, n_exp_pairs, n_cand,
      n_pairs;
  long long first[2];  // per side: the first row, in arrival order, that passes the gate (LMAX: none)
  // of one watermark
  unsigned long long fired[2], n_pad_timer, n_rm_wm;  // fired[c]: a timer of cache c was due (0 / 1)
  // of the handle
  unsigned long long map_full, timers_set;
  long long next_due;  // the earliest set timer (LMAX: none)
  long long active_timers;
  int32_t nslots, pad;
};

struct TMap : KeyMap {
  // per group (slot * 2 + side): the timer that cleans the side's cache (side 0, the left cache: rightTimerState),
  // and a push's first scanning / first cached row of the group (NONE outside a push)
  int64_t* tmr;
  uint32_t *fs, *fc;
};

struct TRows {  // the row store, or a run of rows to merge into it
  uint32_t* g;
  int64_t *ts, *ord, *val;
  uint8_t* emit;
  int64_t cap;
};

struct TOut {
  int64_t *key, *lord, *rord, *lts, *rts, *lval, *rval, *cause, *tts;
};

// A counting kernel runs a bounded grid whose threads stride over the rows and keep their counts in registers: one
// atomic per wave and counter at the end, not one per 64 rows (every wave's add lands on the same address)
constexpr int TJ_COUNT_GRID = 2048;
__device__ __forceinline__ void wave_add(unsigned long long* dst, unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}
// first index of the run (sorted by (g, ts)) whose (g, ts) is >= (kg, kt)
__device__ __forceinline__ int64_t tj_lb(const uint32_t* __restrict__ g, const int64_t* __restrict__ ts, int64_t n,
                                         uint32_t kg, int64_t kt) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const uint32_t gm = g[mid];
    if (gm < kg || (gm == kg && ts[mid] < kt)) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// first index whose (g, ts) is > (kg, kt)
__device__ __forceinline__ int64_t tj_ub(const uint32_t* __restrict__ g, const int64_t* __restrict__ ts, int64_t n,
                                         uint32_t kg, int64_t kt) {
  return kt == LMAX ? tj_lb(g, ts, n, kg + 1, LMIN) : tj_lb(g, ts, n, kg, kt + 1);
}

// ---------------------------------------------------------------- push: check and classify
__global__ void k_tj_reset(TCtr* ctr) {
  ctr->bad_time = ctr->bad_kg = ctr->bad_side = ctr->n_cached = ctr->n_scan = ctr->n_pad_arr = ctr->n_pad_scan = 0;
  ctr->n_rm = ctr->n_exp_pairs = ctr->n_cand = ctr->n_pairs = 0;
  ctr->first[0] = ctr->first[1] = LMAX;
}
// refusals of a whole push, and the gate: per side the first row whose upper bound the other cache's expiration time
// (as the push finds it) has not passed
__global__ __launch_bounds__(256) void k_tj_check(TCfg c, TEpoch ep, const uint8_t* __restrict__ side,
                                                  const int64_t* __restrict__ key, const int64_t* __restrict__ ts,
                                                  const int32_t* __restrict__ kh, int64_t n, TCtr* ctr) {
  unsigned long long a = 0, b = 0, d = 0;
  int64_t f0 = LMAX, f1 = LMAX;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int sd = side[i];
    const int s = sd & 1;
    const int64_t t = ts[i];
    const bool bad_t = t < 0 || t >= TJ_TS_END;
    const int32_t kg = key_group(key_hash_of(c.key_kind, key[i], kh, i), c.max_par);
    a += bad_t ? 1 : 0;
    b += (kg < c.kg0 || kg >= c.kg0 + c.nkg) ? 1 : 0;
    d += sd > 1 ? 1 : 0;
    if (!bad_t && ep.X[1 - s] < t + c.rel[s]) {  // (a thread's rows come in rising order: the first one stays)
      if (s == 0 && f0 == LMAX) f0 = i;
      if (s == 1 && f1 == LMAX) f1 = i;
    }
  }
  wave_add(&ctr->bad_time, a);
  wave_add(&ctr->bad_kg, b);
  wave_add(&ctr->bad_side, d);
  f0 = wave_min64(f0);
  f1 = wave_min64(f1);
  if ((threadIdx.x & 63) == 0) {
    if (f0 != LMAX) atomicMin(&ctr->first[0], (long long)f0);
    if (f1 != LMAX) atomicMin(&ctr->first[1], (long long)f1);
  }
}
// per row: its group, whether it is cached and whether it scans; the radix sort's first key (row time)
__global__ __launch_bounds__(256) void k_tj_classify(TCfg c, TEpoch ep, TMap m, TCtr* ctr,
                                                     const uint8_t* __restrict__ side, const int64_t* __restrict__ key,
                                                     const int64_t* __restrict__ ts, const int32_t* __restrict__ kh,
                                                     int64_t n, uint32_t* __restrict__ pg, uint8_t* __restrict__ pflag,
                                                     uint64_t* __restrict__ k1, uint32_t* __restrict__ v1) {
  unsigned long long a = 0, b = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    bool cached = false, scans = false;
    const int s = side[i] & 1, o = 1 - s;
    const int64_t t = ts[i], k = key[i];
    const int64_t ub = jadd(t, c.rel[s]);
    const int32_t slot = keymap_claim(m, &ctr->nslots, &ctr->map_full, k, [&] { return key_group(key_hash_of(c.key_kind, k, kh, i), c.max_par); });
    uint32_t g = 0;
    if (slot >= 0) {
      g = (uint32_t)slot * 2u + (uint32_t)s;
      cached = ep.T < ub;
      const int64_t f = ctr->first[s];
      scans = i == f || (i > f && ep.E[o] < ub);
      // (the values only fall: a plain read that is already lower spares a hot group's atomic)
      if (scans && m.fs[g] > (uint32_t)i) atomicMin(&m.fs[g], (uint32_t)i);
      if (cached && m.fc[g] > (uint32_t)i) atomicMin(&m.fc[g], (uint32_t)i);
    }
    pg[i] = g;
    pflag[i] = (uint8_t)((cached ? 1 : 0) | (scans ? 2 : 0));
    k1[i] = (uint64_t)t;
    v1[i] = (uint32_t)i;
    a += cached ? 1 : 0;
    b += scans ? 1 : 0;
  }
  wave_add(&ctr->n_cached, a);
  wave_add(&ctr->n_scan, b);
}
__global__ __launch_bounds__(256) void k_tj_key2(const uint32_t* __restrict__ pg, const uint32_t* __restrict__ v, int64_t n,
                                                 uint32_t* __restrict__ k2) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) k2[j] = pg[v[j]];
}
// the batch in (group, row time, ordinal) order
__global__ __launch_bounds__(256) void k_tj_gather(const uint32_t* __restrict__ perm, const int64_t* __restrict__ ts,
                                                   const int64_t* __restrict__ val, const uint8_t* __restrict__ pflag,
                                                   int64_t n, int64_t* __restrict__ sts, int64_t* __restrict__ sval,
                                                   uint8_t* __restrict__ sflag) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = perm[j];
  sts[j] = ts[i];
  sval[j] = val ? val[i] : 0;
  sflag[j] = pflag[i];
}

// ---------------------------------------------------------------- push: partner ranges
// per sorted batch row that scans: its partners in the store [sa, sa + sn) and among the batch's cached rows
// from ba on (those that arrived earlier are its pairs), and the candidate count of both
__global__ __launch_bounds__(256) void k_tj_ranges(TCfg c, TEpoch ep, TMap m, TRows st, int64_t ns,
                                                   const uint32_t* __restrict__ sg, const int64_t* __restrict__ sts,
                                                   const uint32_t* __restrict__ sidx, const uint8_t* __restrict__ sflag,
                                                   int64_t n, uint32_t* __restrict__ sa, uint32_t* __restrict__ sn,
                                                   uint32_t* __restrict__ ba,
                                                   unsigned long long* __restrict__ cnt, TCtr* ctr) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  uint32_t a0 = 0, n0 = 0, a1 = 0, n1 = 0;
  if (sflag[j] & 2) {
    const uint32_t g = sg[j], og = g ^ 1u;
    const int s = (int)(g & 1u), o = 1 - s;
    const int64_t t = sts[j];
    const int64_t lo_t = jsub(t, c.rel[o]), hi_t = jadd(t, c.rel[s]);
    int64_t a = tj_lb(st.g, st.ts, ns, og, lo_t);
    int64_t b = tj_ub(st.g, st.ts, ns, og, hi_t);
    if (b < a) b = a;
    // rows <= the expiration time leave with the group's first scanner: only it sees them
    int64_t e = tj_ub(st.g, st.ts, ns, og, ep.E[o]);
    e = e < a ? a : (e > b ? b : e);
    if (m.fs[g] == sidx[j]) {
      if (e > a) atomicAdd(&ctr->n_exp_pairs, (unsigned long long)(e - a));
    } else {
      a = e;
    }
    a0 = (uint32_t)a;
    n0 = (uint32_t)(b - a);
    // the other side's rows of this push that are cached: row time > T - rel
    const int64_t cmin = ep.T - c.rel[o] + 1;
    const int64_t blo = lo_t > cmin ? lo_t : cmin;
    const int64_t p = tj_lb(sg, sts, n, og, blo);
    int64_t q = tj_ub(sg, sts, n, og, hi_t);
    if (q < p) q = p;
    a1 = (uint32_t)p;
    n1 = (uint32_t)(q - p);
  }
  sa[j] = a0;
  sn[j] = n0;
  ba[j] = a1;
  cnt[j] = (unsigned long long)n0 + n1;
}
__global__ void k_tj_total(const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ off,
                           int64_t n, unsigned long long* dst) {
  *dst = n ? off[n - 1] + cnt[n - 1] : 0ull;
}

// ---------------------------------------------------------------- push: the load-balanced pair pass
// rank of the lanes with `v` among the workgroup's (TJ_THREADS = 4 waves), and their number
__device__ __forceinline__ uint32_t block_rank(bool v, uint32_t* lds, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long b = __ballot(v);
  const uint32_t r = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) lds[w] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t base = 0;
  total = 0;
  for (int q = 0; q < TJ_THREADS / 64; q++) {
    const uint32_t x = lds[q];
    if (q < w) base += x;
    total += x;
  }
  __syncthreads();
  return base + r;
}
// The candidate index space [0, n_cand) is cut into TJ_GRID contiguous spans (a multiple of TJ_CHUNK each); a
// workgroup walks its span in steps of TJ_CHUNK.  Per step two searches in the scanned offsets bound the probe rows
// the step touches; a lane finds its candidate's probe row between them.  EMIT = false: counts the span's pairs and
// marks the joined flags in scratch (bemit: the batch's rows, smark: the store's).  EMIT = true: writes the pairs at
// the span's scanned base, in candidate order.
template <bool EMIT>
__global__ __launch_bounds__(TJ_THREADS) void k_tj_pairs(
    TCfg c, TMap m, TRows st, const uint32_t* __restrict__ sg, const int64_t* __restrict__ sts,
    const uint32_t* __restrict__ sidx, const int64_t* __restrict__ sval, int64_t n, const uint32_t* __restrict__ sa,
    const uint32_t* __restrict__ sn, const uint32_t* __restrict__ ba, const unsigned long long* __restrict__ off,
    const TCtr* __restrict__ ctr, uint8_t* __restrict__ bemit, uint8_t* __restrict__ smark,
    unsigned long long* __restrict__ wgcnt, const unsigned long long* __restrict__ wgoff, TOut out, int64_t obase,
    int64_t ord_base) {
  __shared__ uint32_t lds[TJ_THREADS / 64];
  __shared__ int64_t jb[2];
  __shared__ unsigned long long red[TJ_THREADS / 64];
  const unsigned long long total = ctr->n_cand;
  unsigned long long per = (total + TJ_GRID - 1) / TJ_GRID;
  per = (per + TJ_CHUNK - 1) / TJ_CHUNK * TJ_CHUNK;
  const unsigned long long start = (unsigned long long)blockIdx.x * per;
  const unsigned long long end = start + per < total ? start + per : total;
  if (start >= end) {
    if (!EMIT && threadIdx.x == 0) wgcnt[blockIdx.x] = 0;
    return;
  }
  unsigned long long mine = 0;                                      // !EMIT: this lane's pairs
  int64_t dst = EMIT ? obase + (int64_t)wgoff[blockIdx.x] : 0;       // EMIT: the next output row of the span
  for (unsigned long long c0 = start; c0 < end; c0 += TJ_CHUNK) {
    const unsigned long long c1 = c0 + TJ_CHUNK < end ? c0 + TJ_CHUNK : end;
    if (threadIdx.x < 2) {  // the last probe row whose offset is <= the step's first / last candidate
      const unsigned long long x = threadIdx.x == 0 ? c0 : c1 - 1;
      int64_t lo = 0, hi = n - 1;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= x) lo = mid; else hi = mid - 1;
      }
      jb[threadIdx.x] = lo;
    }
    __syncthreads();
    const int64_t jlo = jb[0], jhi = jb[1];
    for (int k = 0; k < TJ_ITEMS; k++) {
      const unsigned long long idx = c0 + (unsigned long long)k * TJ_THREADS + threadIdx.x;
      bool valid = false;
      int64_t j = 0, ps = -1, pb = -1;
      if (idx < c1) {
        int64_t lo = jlo, hi = jhi;
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo + 1) >> 1);
          if (off[mid] <= idx) lo = mid; else hi = mid - 1;
        }
        j = lo;
        const unsigned long long r = idx - off[j];
        if (r < sn[j]) {
          ps = (int64_t)sa[j] + (int64_t)r;
          valid = true;
        } else {
          pb = (int64_t)ba[j] + (int64_t)(r - sn[j]);
          valid = sidx[pb] < sidx[j];  // emitted by the later of the two
        }
      }
      if (!EMIT) {
        if (valid) {
          mine++;
          bemit[j] = 1;
          if (tj_pads(c.type, 1 - (int)(sg[j] & 1u))) {
            if (ps >= 0) smark[ps] = 1; else bemit[pb] = 1;
          }
        }
      } else {
        uint32_t tot;
        const uint32_t rk = block_rank(valid, lds, tot);
        if (valid) {
          const int64_t d = dst + rk;
          const uint32_t g = sg[j];
          const int s = (int)(g & 1u);
          const int64_t o_ord = ord_base + sidx[j], o_ts = sts[j], o_val = sval[j];
          int64_t p_ord, p_ts, p_val;
          if (ps >= 0) {
            p_ord = st.ord[ps];
            p_ts = st.ts[ps];
            p_val = st.val[ps];
          } else {
            p_ord = ord_base + sidx[pb];
            p_ts = sts[pb];
            p_val = sval[pb];
          }
          out.key[d] = m.skey[g >> 1];
          out.lord[d] = s == 0 ? o_ord : p_ord;
          out.rord[d] = s == 0 ? p_ord : o_ord;
          out.lts[d] = s == 0 ? o_ts : p_ts;
          out.rts[d] = s == 0 ? p_ts : o_ts;
          out.lval[d] = s == 0 ? o_val : p_val;
          out.rval[d] = s == 0 ? p_val : o_val;
          out.cause[d] = o_ord;
          out.tts[d] = -1;
        }
        dst += tot;
      }
    }
    __syncthreads();  // jb is rewritten by the next step
  }
  if (!EMIT) {
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = 0;
      for (int q = 0; q < TJ_THREADS / 64; q++) t += red[q];
      wgcnt[blockIdx.x] = t;
    }
  }
}

// ---------------------------------------------------------------- push: padding, removal, merge, timers
// a row that is not cached and joined nothing is padded at once
__global__ __launch_bounds__(256) void k_tj_pad_arr_flags(TCfg c, const uint32_t* __restrict__ sg,
                                                          const uint8_t* __restrict__ sflag,
                                                          const uint8_t* __restrict__ bemit, int64_t n,
                                                          uint32_t* __restrict__ parr, TCtr* ctr) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool p = false;
  if (j < n) {
    p = !(sflag[j] & 1) && !bemit[j] && tj_pads(c.type, (int)(sg[j] & 1u));
    parr[j] = p ? 1u : 0u;
  }
  const unsigned long long a = wave_count(p);
  if ((threadIdx.x & 63) == 0 && a) atomicAdd(&ctr->n_pad_arr, a);
}
// a store row <= the expiration time leaves when the other side's group has a scanner in this push; padded if it was
// never joined
__global__ __launch_bounds__(256) void k_tj_rm_flags(TCfg c, TEpoch ep, TMap m, TRows st, int64_t ns,
                                                     const uint8_t* __restrict__ smark, uint32_t* __restrict__ keep,
                                                     uint32_t* __restrict__ pscan, TCtr* ctr) {
  unsigned long long a = 0, b = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < ns; r += stride) {
    const uint32_t g = st.g[r];
    const int cs = (int)(g & 1u);
    const bool rm = m.fs[g ^ 1u] != NONE && st.ts[r] <= ep.E[cs];
    const bool p = rm && tj_pads(c.type, cs) && !(st.emit[r] | smark[r]);
    keep[r] = rm ? 0u : 1u;
    pscan[r] = p ? 1u : 0u;
    a += rm ? 1 : 0;
    b += p ? 1 : 0;
  }
  wave_add(&ctr->n_rm, a);
  wave_add(&ctr->n_pad_scan, b);
}
__device__ __forceinline__ void tj_write_pad(const TOut& out, int64_t d, int64_t key, int side, int64_t ord, int64_t ts,
                                             int64_t val, int64_t cause, int64_t tts) {
  out.key[d] = key;
  out.lord[d] = side == 0 ? ord : -1;
  out.rord[d] = side == 0 ? -1 : ord;
  out.lts[d] = side == 0 ? ts : 0;
  out.rts[d] = side == 0 ? 0 : ts;
  out.lval[d] = side == 0 ? val : 0;
  out.rval[d] = side == 0 ? 0 : val;
  out.cause[d] = cause;
  out.tts[d] = tts;
}
__global__ __launch_bounds__(256) void k_tj_pad_arr(TMap m, const uint32_t* __restrict__ sg, const int64_t* __restrict__ sts,
                                                    const uint32_t* __restrict__ sidx, const int64_t* __restrict__ sval,
                                                    int64_t n, const uint32_t* __restrict__ parr,
                                                    const uint32_t* __restrict__ ppos, TOut out, int64_t obase,
                                                    int64_t ord_base) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || !parr[j]) return;
  const uint32_t g = sg[j];
  const int64_t ord = ord_base + sidx[j];
  tj_write_pad(out, obase + ppos[j], m.skey[g >> 1], (int)(g & 1u), ord, sts[j], sval[j], ord, -1);
}
// timer == false: padded by the scanning row that met it; true: by the group's clean-up timer
__global__ __launch_bounds__(256) void k_tj_pad_store(TMap m, TRows st, int64_t ns, const uint32_t* __restrict__ pf,
                                                      const uint32_t* __restrict__ ppos, TOut out, int64_t obase,
                                                      int64_t ord_base, bool timer) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ns || !pf[r]) return;
  const uint32_t g = st.g[r];
  const int64_t cause = timer ? -1 : ord_base + m.fs[g ^ 1u];
  tj_write_pad(out, obase + ppos[r], m.skey[g >> 1], (int)(g & 1u), st.ord[r], st.ts[r], st.val[r], cause,
               timer ? m.tmr[g] : -1);
}
// the batch's cached rows, in order, as a run to merge
__global__ __launch_bounds__(256) void k_tj_cached_flags(const uint8_t* __restrict__ sflag, int64_t n, uint32_t* __restrict__ cf) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) cf[j] = sflag[j] & 1u;
}
__global__ __launch_bounds__(256) void k_tj_cached_run(const uint32_t* __restrict__ sg, const int64_t* __restrict__ sts,
                                                       const uint32_t* __restrict__ sidx, const int64_t* __restrict__ sval,
                                                       const uint8_t* __restrict__ bemit, int64_t n,
                                                       const uint32_t* __restrict__ cf, const uint32_t* __restrict__ cpos,
                                                       TRows run, int64_t ord_base) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || !cf[j]) return;
  const int64_t d = cpos[j];
  if (d >= run.cap) return;
  run.g[d] = sg[j];
  run.ts[d] = sts[j];
  run.ord[d] = ord_base + sidx[j];
  run.val[d] = sval[j];
  run.emit[d] = bemit[j];
}
// merge of two sorted runs into `dst`: the store's kept rows (kpos: their rank among themselves) and `run` (m rows,
// none equal to a store row in (group, row time, ordinal); on equal (group, row time) the store's row is the earlier)
__global__ __launch_bounds__(256) void k_tj_merge_old(TRows st, int64_t ns, const uint32_t* __restrict__ keep,
                                                      const uint32_t* __restrict__ kpos, const uint8_t* __restrict__ smark,
                                                      TRows run, int64_t m, TRows dst) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ns || !keep[r]) return;
  const uint32_t g = st.g[r];
  const int64_t t = st.ts[r];
  const int64_t d = (int64_t)kpos[r] + tj_lb(run.g, run.ts, m, g, t);
  if (d >= dst.cap) return;
  dst.g[d] = g;
  dst.ts[d] = t;
  dst.ord[d] = st.ord[r];
  dst.val[d] = st.val[r];
  dst.emit[d] = st.emit[r] | smark[r];
}
__global__ __launch_bounds__(256) void k_tj_merge_new(TRows st, int64_t ns, const uint32_t* __restrict__ kpos,
                                                      int64_t nkept, TRows run, int64_t m, TRows dst) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m) return;
  const uint32_t g = run.g[q];
  const int64_t t = run.ts[q];
  const int64_t u = tj_ub(st.g, st.ts, ns, g, t);
  const int64_t d = q + (u < ns ? (int64_t)kpos[u] : nkept);
  if (d >= dst.cap) return;
  dst.g[d] = g;
  dst.ts[d] = t;
  dst.ord[d] = run.ord[q];
  dst.val[d] = run.val[q];
  dst.emit[d] = run.emit[q];
}
// a push that neither removes nor caches a row still joins cached ones: their flags
__global__ __launch_bounds__(256) void k_tj_or_marks(TRows st, int64_t ns, const uint8_t* __restrict__ smark) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < ns && smark[r]) st.emit[r] = 1;
}
// a group's timer that is unset is armed by the group's first cached row in arrival order
__global__ __launch_bounds__(256) void k_tj_arm(TCfg c, TMap m, const uint32_t* __restrict__ sg, const int64_t* __restrict__ sts,
                                                const uint32_t* __restrict__ sidx, const uint8_t* __restrict__ sflag,
                                                int64_t n, TCtr* ctr) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || !(sflag[j] & 1)) return;
  const uint32_t g = sg[j];
  if (m.fc[g] != sidx[j] || m.tmr[g] != 0) return;
  const int64_t t = sts[j] + c.rel[g & 1u] + c.M + c.L + 1;
  m.tmr[g] = t;
  atomicMin(&ctr->next_due, (long long)t);
  atomicAdd(&ctr->timers_set, 1ull);
  atomicAdd((unsigned long long*)&ctr->active_timers, 1ull);
}
__global__ __launch_bounds__(256) void k_tj_unmark(TMap m, const uint32_t* __restrict__ pg, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = pg[i];
  if (g >= 2u * (uint32_t)m.max_keys) return;
  m.fs[g] = NONE;
  m.fc[g] = NONE;
}

// ---------------------------------------------------------------- watermark
__global__ __launch_bounds__(256) void k_tj_due(TMap m, int64_t ng, int64_t wm, uint8_t* __restrict__ due,
                                                int64_t* __restrict__ tnew, uint8_t* __restrict__ clr, TCtr* ctr) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) {
    ctr->next_due = LMAX;
    ctr->n_pad_timer = ctr->n_rm_wm = 0;
  }
  if (g >= ng) return;
  const int64_t t = m.tmr[g];
  const bool d = t != 0 && t <= wm;
  due[g] = d ? 1 : 0;
  tnew[g] = 0;
  clr[g] = 0;
  if (d) ctr->fired[g & 1] = 1;  // (a flag: every writer stores the same value)
}
// the first remaining row of a due run: the new timer, or, at row time 0, the whole run is cleared without padding
__global__ __launch_bounds__(256) void k_tj_wm_first(TCfg c, TEpoch ep, TRows st, int64_t ns, const uint8_t* __restrict__ due,
                                                     int64_t* __restrict__ tnew, uint8_t* __restrict__ clr) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ns) return;
  const uint32_t g = st.g[r];
  if (!due[g]) return;
  const int cs = (int)(g & 1u);
  const int64_t t = st.ts[r];
  if (t <= ep.E[cs]) return;
  if (r > 0 && st.g[r - 1] == g && st.ts[r - 1] > ep.E[cs]) return;
  if (t > 0) tnew[g] = t + c.rel[cs] + c.M + c.L + 1; else clr[g] = 1;
}
__global__ __launch_bounds__(256) void k_tj_wm_flags(TCfg c, TEpoch ep, TRows st, int64_t ns, const uint8_t* __restrict__ due,
                                                     const uint8_t* __restrict__ clr, uint32_t* __restrict__ keep,
                                                     uint32_t* __restrict__ pad, TCtr* ctr) {
  unsigned long long a = 0, b = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < ns; r += stride) {
    bool rm = false, p = false;
    const uint32_t g = st.g[r];
    const int cs = (int)(g & 1u);
    if (due[g]) {
      const bool expired = st.ts[r] <= ep.E[cs];
      rm = expired || clr[g];
      p = expired && !st.emit[r] && tj_pads(c.type, cs);
    }
    keep[r] = rm ? 0u : 1u;
    pad[r] = p ? 1u : 0u;
    a += rm ? 1 : 0;
    b += p ? 1 : 0;
  }
  wave_add(&ctr->n_rm_wm, a);
  wave_add(&ctr->n_pad_timer, b);
}
__global__ __launch_bounds__(256) void k_tj_compact(TRows st, int64_t ns, const uint32_t* __restrict__ keep,
                                                    const uint32_t* __restrict__ kpos, TRows dst) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ns || !keep[r]) return;
  const int64_t d = kpos[r];
  dst.g[d] = st.g[r];
  dst.ts[d] = st.ts[r];
  dst.ord[d] = st.ord[r];
  dst.val[d] = st.val[r];
  dst.emit[d] = st.emit[r];
}
// the due timers' new values, and the earliest set timer over all groups
__global__ __launch_bounds__(256) void k_tj_wm_timers(TMap m, int64_t ng, const uint8_t* __restrict__ due,
                                                      const int64_t* __restrict__ tnew, TCtr* ctr) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t t = LMAX;
  bool set = false, gone = false;
  if (g < ng) {
    int64_t v = m.tmr[g];
    if (due[g]) {
      v = tnew[g];
      m.tmr[g] = v;
      set = v != 0;
      gone = v == 0;
    }
    if (v != 0) t = v;
  }
  t = wave_min64(t);
  const unsigned long long a = wave_count(set), b = wave_count(gone);
  if ((threadIdx.x & 63) == 0) {
    if (t != LMAX) atomicMin(&ctr->next_due, (long long)t);
    if (a) atomicAdd(&ctr->timers_set, a);
    if (b) atomicAdd((unsigned long long*)&ctr->active_timers, (unsigned long long)(-(long long)b));
  }
}

// ---------------------------------------------------------------- restore
__global__ __launch_bounds__(256) void k_tj_restore_keys(TCfg c, TMap m, TCtr* ctr, int32_t kg, const int64_t* __restrict__ key,
                                                         const int64_t* __restrict__ lt, const int64_t* __restrict__ rt,
                                                         int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t slot = keymap_claim(m, &ctr->nslots, &ctr->map_full, key[i], [&] { return kg; });
  if (slot < 0) return;
  m.skg[slot] = kg;
  // leftTimerState cleans the right cache (side 1), rightTimerState the left
  const int64_t tv[2] = {rt[i], lt[i]};
  for (int s = 0; s < 2; s++) {
    m.tmr[(int64_t)slot * 2 + s] = tv[s];
    if (tv[s] != 0) {
      atomicMin(&ctr->next_due, (long long)tv[s]);
      atomicAdd((unsigned long long*)&ctr->active_timers, 1ull);
    }
  }
}
__global__ __launch_bounds__(256) void k_tj_restore_groups(TMap m, const int64_t* __restrict__ key, const uint8_t* __restrict__ side,
                                                           int64_t n, uint32_t* __restrict__ k2, uint32_t* __restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t slot = keymap_find(m, key[i]);
  k2[i] = slot < 0 ? 0u : (uint32_t)slot * 2u + (side[i] & 1u);
  v[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_tj_restore_run(const uint32_t* __restrict__ g, const uint32_t* __restrict__ perm,
                                                        const int64_t* __restrict__ ts, const int64_t* __restrict__ ord,
                                                        const int64_t* __restrict__ val, const uint8_t* __restrict__ emit,
                                                        int64_t n, TRows run) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = perm[j];
  run.g[j] = g[j];
  run.ts[j] = ts[i];
  run.ord[j] = ord[i];
  run.val[j] = val[i];
  run.emit[j] = emit[i];
}
__global__ __launch_bounds__(256) void k_tj_iota(uint32_t* keep, uint32_t* kpos, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keep[i] = 1u;
  kpos[i] = (uint32_t)i;
}

}  // namespace

struct fw_tjoin : TableHandle {  // (oseg's epochs: the watermark calls so far)
  fw_tjoin_config cfg{};
  TCfg c{};
  TMap map{};
  TCtr* ctr = nullptr;   // device
  TCtr* hctr = nullptr;  // pinned host copy
  TRows store[2]{}, run{};
  int cur = 0;
  int64_t n_store = 0, nslots = 0;
  int64_t wm = LMIN, next_due = LMAX, ord_base = 0, wm_calls = 0;
  bool due_dirty = false;  // a push or restore may have armed a timer since next_due was read
  int64_t X[2] = {0, 0};   // leftExpirationTime, rightExpirationTime
  int64_t rows_in = 0, cached = 0, not_cached = 0, pairs = 0, pad_arr = 0, pad_scan = 0, pad_timer = 0, exp_pairs = 0,
          gate_skips = 0;
  TOut out{};
  int64_t max_rows = 0;
  Buf b_stage[5], b_pg, b_pflag, b_k1[2], b_v1[2], b_k2[2], b_v2, b_sts, b_sval, b_sflag, b_sa, b_sn, b_ba,
      b_cnt, b_off, b_bemit, b_smark, b_wgcnt, b_wgoff, b_parr, b_ppos, b_keep, b_kpos, b_pscan, b_spos, b_cf, b_cpos,
      b_due, b_tnew, b_clr;
};

namespace {

// the column sets: the row store (and a run to merge), a key slot's state, the output
Cols row_cols(TRows& r) { return Cols{col(r.g), col(r.ts), col(r.ord), col(r.val), col(r.emit)}; }
Cols slot_cols(TMap& m) {  // (besides the key map's own skey, skg) two groups per slot; fs, fc: NONE outside a push
  return Cols{col(m.tmr, 16, 1, 0), col(m.fs, 8, 1, 0xFF), col(m.fc, 8, 1, 0xFF)};
}
Cols out_cols(TOut& o) {
  return Cols{col(o.key), col(o.lord), col(o.rord), col(o.lts), col(o.rts), col(o.lval), col(o.rval), col(o.cause), col(o.tts)};
}

int grow_store(fw_tjoin* op, int64_t need) { return grow_store(op, op->store, op->cur, op->n_store, need, row_cols); }
int grow_run(fw_tjoin* op, int64_t need) {  // (contents are not kept)
  if (need <= op->run.cap) return FW_OK;
  const int rc = settle(op);
  return rc ? rc : cols_grow(op, op->run, op->run.cap, need, 0, row_cols, "cannot allocate a row store of %lld rows");
}
int grow_map(fw_tjoin* op, int64_t keys) { return grow_map(op, op->map, op->nslots, keys, 29, slot_cols); }
int grow_out(fw_tjoin* op, int64_t need) {
  return cols_grow(op, op->out, op->ocap, need, op->n_out, out_cols, "cannot allocate an output buffer of %lld rows");
}
unsigned group_bits(const fw_tjoin* op) {
  unsigned b = 1;
  while ((int64_t(1) << b) < 2 * (int64_t)op->map.max_keys) b++;
  return b;
}

TEpoch epoch_of(const fw_tjoin* op, int64_t wm) {
  TEpoch ep;
  const int64_t T = wm > 0 ? wm : 0;
  ep.T = std::min(T, TJ_T_CLAMP);
  for (int s = 0; s < 2; s++) {
    ep.E[s] = T == LMAX ? LMAX : ep.T - op->c.rel[s] - op->c.L - 1;  // calExpirationTime
    ep.X[s] = op->X[s];
  }
  return ep;
}

#define TJ_U32(b) ((uint32_t*)(b).p)
#define TJ_U8(b) ((uint8_t*)(b).p)
#define TJ_I64(b) ((int64_t*)(b).p)
#define TJ_U64(b) ((unsigned long long*)(b).p)

// the store's kept rows (b_keep / b_kpos / b_smark, nkept of them) and op->run's m rows become the other store buffer
int merge_run(fw_tjoin* op, int64_t nkept, int64_t m) {
  const TRows& st = op->store[op->cur];
  const TRows& dst = op->store[op->cur ^ 1];
  const int64_t ns = op->n_store;
  if (ns)
    hipLaunchKernelGGL(k_tj_merge_old, dim3(grid_of(ns)), dim3(256), 0, op->stream, st, ns, TJ_U32(op->b_keep),
                       TJ_U32(op->b_kpos), TJ_U8(op->b_smark), op->run, m, dst);
  if (m)
    hipLaunchKernelGGL(k_tj_merge_new, dim3(grid_of(m)), dim3(256), 0, op->stream, st, ns, TJ_U32(op->b_kpos), nkept,
                       op->run, m, dst);
  op->cur ^= 1;
  op->n_store = nkept + m;
  return FW_OK;
}

int do_push(fw_tjoin* op, const uint8_t* side, const int64_t* key, const int64_t* ts, const int64_t* val,
            const int32_t* kh, int64_t n) {
  if (n == 0) return FW_OK;
  if (n >= (int64_t(1) << 30)) return set_err(op, FW_ERR_ARG, "a push holds fewer than 2^30 rows");
  const TCfg& c = op->c;
  hipStream_t sm = op->stream;
  int rc;
  // room first: none of it is state
  if ((rc = grow_map(op, op->nslots + n))) return rc;
  if ((rc = grow_store(op, op->n_store + n))) return rc;
  if ((rc = grow_run(op, n))) return rc;
  const int64_t ns = op->n_store;
  const size_t N = (size_t)n, S = (size_t)std::max<int64_t>(ns, 1);
  if ((rc = ensure(op, op->b_pg, N * 4)) || (rc = ensure(op, op->b_pflag, N)) || (rc = ensure(op, op->b_k1[0], N * 8)) ||
      (rc = ensure(op, op->b_k1[1], N * 8)) || (rc = ensure(op, op->b_v1[0], N * 4)) ||
      (rc = ensure(op, op->b_v1[1], N * 4)) || (rc = ensure(op, op->b_k2[0], N * 4)) ||
      (rc = ensure(op, op->b_k2[1], N * 4)) || (rc = ensure(op, op->b_v2, N * 4)) || (rc = ensure(op, op->b_sts, N * 8)) ||
      (rc = ensure(op, op->b_sval, N * 8)) || (rc = ensure(op, op->b_sflag, N)) || (rc = ensure(op, op->b_sa, N * 4)) ||
      (rc = ensure(op, op->b_sn, N * 4)) || (rc = ensure(op, op->b_ba, N * 4)) ||
      (rc = ensure(op, op->b_cnt, N * 8)) || (rc = ensure(op, op->b_off, N * 8)) || (rc = ensure(op, op->b_bemit, N)) ||
      (rc = ensure(op, op->b_smark, S)) || (rc = ensure(op, op->b_wgcnt, TJ_GRID * 8)) ||
      (rc = ensure(op, op->b_wgoff, TJ_GRID * 8)) || (rc = ensure(op, op->b_parr, N * 4)) ||
      (rc = ensure(op, op->b_ppos, N * 4)) || (rc = ensure(op, op->b_keep, S * 4)) || (rc = ensure(op, op->b_kpos, S * 4)) ||
      (rc = ensure(op, op->b_pscan, S * 4)) || (rc = ensure(op, op->b_spos, S * 4)) || (rc = ensure(op, op->b_cf, N * 4)) ||
      (rc = ensure(op, op->b_cpos, N * 4)))
    return rc;
  const TEpoch ep = epoch_of(op, op->wm);
  const TRows& st = op->store[op->cur];
  const unsigned gn = grid_of(n), gs = grid_of(ns);
  uint32_t *sg = nullptr, *sidx = nullptr;

  // ---- count: nothing below changes the handle's state (claimed key slots carry none)
  hipLaunchKernelGGL(k_tj_reset, dim3(1), dim3(1), 0, sm, op->ctr);
  hipLaunchKernelGGL(k_tj_check, dim3(std::min(gn, (unsigned)TJ_COUNT_GRID)), dim3(256), 0, sm, c, ep, side, key, ts, kh, n, op->ctr);
  hipLaunchKernelGGL(k_tj_classify, dim3(std::min(gn, (unsigned)TJ_COUNT_GRID)), dim3(256), 0, sm, c, ep, op->map, op->ctr, side, key, ts, kh, n,
                     TJ_U32(op->b_pg), TJ_U8(op->b_pflag), (uint64_t*)op->b_k1[0].p, TJ_U32(op->b_v1[0]));
  if ((rc = sort_pairs<uint64_t>(op, (const uint64_t*)op->b_k1[0].p, (uint64_t*)op->b_k1[1].p, TJ_U32(op->b_v1[0]),
                                 TJ_U32(op->b_v1[1]), n, 62u)))
    goto unmark;
  hipLaunchKernelGGL(k_tj_key2, dim3(gn), dim3(256), 0, sm, TJ_U32(op->b_pg), TJ_U32(op->b_v1[1]), n, TJ_U32(op->b_k2[0]));
  if ((rc = sort_pairs<uint32_t>(op, TJ_U32(op->b_k2[0]), TJ_U32(op->b_k2[1]), TJ_U32(op->b_v1[1]), TJ_U32(op->b_v2), n,
                                 group_bits(op))))
    goto unmark;
  sg = TJ_U32(op->b_k2[1]);
  sidx = TJ_U32(op->b_v2);
  hipLaunchKernelGGL(k_tj_gather, dim3(gn), dim3(256), 0, sm, sidx, ts, val, TJ_U8(op->b_pflag), n, TJ_I64(op->b_sts),
                     TJ_I64(op->b_sval), TJ_U8(op->b_sflag));
  hipLaunchKernelGGL(k_tj_ranges, dim3(gn), dim3(256), 0, sm, c, ep, op->map, st, ns, sg, TJ_I64(op->b_sts), sidx,
                     TJ_U8(op->b_sflag), n, TJ_U32(op->b_sa), TJ_U32(op->b_sn), TJ_U32(op->b_ba),
                     TJ_U64(op->b_cnt), op->ctr);
  if ((rc = excl_scan<unsigned long long>(op, TJ_U64(op->b_cnt), TJ_U64(op->b_off), n))) goto unmark;
  hipLaunchKernelGGL(k_tj_total, dim3(1), dim3(1), 0, sm, TJ_U64(op->b_cnt), TJ_U64(op->b_off), n, &op->ctr->n_cand);
  if (hipMemsetAsync(op->b_bemit.p, 0, N, sm) != hipSuccess || hipMemsetAsync(op->b_smark.p, 0, S, sm) != hipSuccess) {
    rc = set_err(op, FW_ERR_HIP, "hipMemsetAsync failed");
    goto unmark;
  }
  hipLaunchKernelGGL(k_tj_pairs<false>, dim3(TJ_GRID), dim3(TJ_THREADS), 0, sm, c, op->map, st, sg, TJ_I64(op->b_sts), sidx,
                     TJ_I64(op->b_sval), n, TJ_U32(op->b_sa), TJ_U32(op->b_sn), TJ_U32(op->b_ba), TJ_U64(op->b_off),
                     op->ctr, TJ_U8(op->b_bemit), TJ_U8(op->b_smark), TJ_U64(op->b_wgcnt), TJ_U64(op->b_wgoff), op->out,
                     (int64_t)0, op->ord_base);
  if ((rc = excl_scan<unsigned long long>(op, TJ_U64(op->b_wgcnt), TJ_U64(op->b_wgoff), TJ_GRID))) goto unmark;
  hipLaunchKernelGGL(k_tj_total, dim3(1), dim3(1), 0, sm, TJ_U64(op->b_wgcnt), TJ_U64(op->b_wgoff), (int64_t)TJ_GRID,
                     &op->ctr->n_pairs);
  hipLaunchKernelGGL(k_tj_pad_arr_flags, dim3(gn), dim3(256), 0, sm, c, sg, TJ_U8(op->b_sflag), TJ_U8(op->b_bemit), n,
                     TJ_U32(op->b_parr), op->ctr);
  if (ns)
    hipLaunchKernelGGL(k_tj_rm_flags, dim3(std::min(gs, (unsigned)TJ_COUNT_GRID)), dim3(256), 0, sm, c, ep, op->map, st, ns, TJ_U8(op->b_smark),
                       TJ_U32(op->b_keep), TJ_U32(op->b_pscan), op->ctr);
  // ---- the push's one read
  if ((rc = read_ctr(op))) goto unmark;
  {
    const TCtr& h = *op->hctr;
    op->nslots = h.nslots;
    if (h.map_full) {  // (grow_map made room for every row: unreachable; the handle is unusable from here on)
      op->ready = false;
      rc = set_err(op, FW_ERR_STATE, "the key map overflowed");
    }
    else if (h.bad_side) rc = set_err(op, FW_ERR_ARG, "%llu rows have a side outside {0, 1}; the push was refused", h.bad_side);
    else if (h.bad_time)
      rc = set_err(op, FW_ERR_TIME_RANGE,
                   "%llu rows have a row time outside [0, 2^62); the push was refused", h.bad_time);
    else if (h.bad_kg) rc = set_err(op, FW_ERR_KEY_GROUP, "%llu rows have a key outside KeyGroupRange [%d, %d]; the push was refused",
                                    h.bad_kg, c.kg0, c.kg0 + c.nkg - 1);
    if (rc) goto unmark;
    const int64_t npairs = (int64_t)h.n_pairs, npa = (int64_t)h.n_pad_arr, nps = (int64_t)h.n_pad_scan;
    const int64_t nrm = (int64_t)h.n_rm, ncached = (int64_t)h.n_cached;
    const int64_t nrows = npairs + npa + nps;
    if (op->n_out + nrows > op->max_rows) {
      rc = set_err(op, FW_ERR_CAPACITY, "%lld pending rows and the push's %lld rows exceed max_pairs = %lld; drain first",
                   (long long)op->n_out, (long long)nrows, (long long)op->max_rows);
      goto unmark;
    }
    if ((rc = grow_out(op, op->n_out + nrows))) goto unmark;
    // ---- commit
    const int64_t ob = op->n_out;
    if (npairs)
      hipLaunchKernelGGL(k_tj_pairs<true>, dim3(TJ_GRID), dim3(TJ_THREADS), 0, sm, c, op->map, st, sg, TJ_I64(op->b_sts),
                         sidx, TJ_I64(op->b_sval), n, TJ_U32(op->b_sa), TJ_U32(op->b_sn), TJ_U32(op->b_ba),
                         TJ_U64(op->b_off), op->ctr, TJ_U8(op->b_bemit), TJ_U8(op->b_smark), TJ_U64(op->b_wgcnt),
                         TJ_U64(op->b_wgoff), op->out, ob, op->ord_base);
    if (npa) {
      if ((rc = excl_scan<uint32_t>(op, TJ_U32(op->b_parr), TJ_U32(op->b_ppos), n))) goto broken;
      hipLaunchKernelGGL(k_tj_pad_arr, dim3(gn), dim3(256), 0, sm, op->map, sg, TJ_I64(op->b_sts), sidx,
                         TJ_I64(op->b_sval), n, TJ_U32(op->b_parr), TJ_U32(op->b_ppos), op->out, ob + npairs, op->ord_base);
    }
    if (nps) {
      if ((rc = excl_scan<uint32_t>(op, TJ_U32(op->b_pscan), TJ_U32(op->b_spos), ns))) goto broken;
      hipLaunchKernelGGL(k_tj_pad_store, dim3(gs), dim3(256), 0, sm, op->map, st, ns, TJ_U32(op->b_pscan),
                         TJ_U32(op->b_spos), op->out, ob + npairs + npa, op->ord_base, false);
    }
    if (ns && (rc = excl_scan<uint32_t>(op, TJ_U32(op->b_keep), TJ_U32(op->b_kpos), ns))) goto broken;
    if (ncached) {
      hipLaunchKernelGGL(k_tj_cached_flags, dim3(gn), dim3(256), 0, sm, TJ_U8(op->b_sflag), n, TJ_U32(op->b_cf));
      if ((rc = excl_scan<uint32_t>(op, TJ_U32(op->b_cf), TJ_U32(op->b_cpos), n))) goto broken;
    }
    if (ncached) hipLaunchKernelGGL(k_tj_cached_run, dim3(gn), dim3(256), 0, sm, sg, TJ_I64(op->b_sts), sidx, TJ_I64(op->b_sval),
                       TJ_U8(op->b_bemit), n, TJ_U32(op->b_cf), TJ_U32(op->b_cpos), op->run, op->ord_base);
    if (nrm || ncached) merge_run(op, ns - nrm, ncached);
    else if (ns && npairs) hipLaunchKernelGGL(k_tj_or_marks, dim3(gs), dim3(256), 0, sm, st, ns, TJ_U8(op->b_smark));
    hipLaunchKernelGGL(k_tj_arm, dim3(gn), dim3(256), 0, sm, c, op->map, sg, TJ_I64(op->b_sts), sidx, TJ_U8(op->b_sflag), n,
                       op->ctr);
    hipLaunchKernelGGL(k_tj_unmark, dim3(gn), dim3(256), 0, sm, op->map, TJ_U32(op->b_pg), n);
    for (int s = 0; s < 2; s++)
      if (h.first[s] != LMAX) op->X[1 - s] = ep.E[1 - s];  // a row of side s passed the gate: the other cache's time
    op->n_out += nrows;
    append_segment(op, op->wm_calls, nrows);
    op->rows_in += n;
    op->ord_base += n;
    op->cached += ncached;
    op->not_cached += n - ncached;
    op->pairs += npairs;
    op->pad_arr += npa;
    op->pad_scan += nps;
    op->exp_pairs += (int64_t)h.n_exp_pairs;
    op->gate_skips += n - (int64_t)h.n_scan;
    op->due_dirty = true;
    return FW_OK;
  }
broken:
  op->ready = false;  // a failure after the commit began
  return rc;
unmark:
  hipLaunchKernelGGL(k_tj_unmark, dim3(gn), dim3(256), 0, sm, op->map, TJ_U32(op->b_pg), n);
  (void)hipStreamSynchronize(sm);
  return rc;
}

int do_watermark(fw_tjoin* op, int64_t wm, int64_t* n_rows) {
  int rc;
  if (n_rows) *n_rows = 0;
  if (op->due_dirty) {
    if ((rc = read_ctr(op))) return rc;
    op->next_due = op->hctr->next_due;
    op->due_dirty = false;
  }
  const int64_t call = op->wm_calls++;
  op->wm = wm;
  if (wm < op->next_due) return FW_OK;
  const TCfg& c = op->c;
  hipStream_t sm = op->stream;
  const TEpoch ep = epoch_of(op, wm);
  const int64_t ns = op->n_store, ng = 2 * op->nslots;
  const size_t S = (size_t)std::max<int64_t>(ns, 1), G = (size_t)std::max<int64_t>(ng, 1);
  if ((rc = ensure(op, op->b_due, G)) || (rc = ensure(op, op->b_tnew, G * 8)) || (rc = ensure(op, op->b_clr, G)) ||
      (rc = ensure(op, op->b_keep, S * 4)) || (rc = ensure(op, op->b_kpos, S * 4)) || (rc = ensure(op, op->b_pscan, S * 4)) ||
      (rc = ensure(op, op->b_spos, S * 4)))
    return rc;
  const TRows& st = op->store[op->cur];
  const unsigned gs = grid_of(ns), gg = grid_of(ng);
  TB_HIP(op, hipMemsetAsync(&op->ctr->fired[0], 0, 16, sm));
  hipLaunchKernelGGL(k_tj_due, dim3(gg), dim3(256), 0, sm, op->map, ng, wm, TJ_U8(op->b_due), TJ_I64(op->b_tnew),
                     TJ_U8(op->b_clr), op->ctr);
  if (ns) {
    hipLaunchKernelGGL(k_tj_wm_first, dim3(gs), dim3(256), 0, sm, c, ep, st, ns, TJ_U8(op->b_due), TJ_I64(op->b_tnew),
                       TJ_U8(op->b_clr));
    hipLaunchKernelGGL(k_tj_wm_flags, dim3(std::min(gs, (unsigned)TJ_COUNT_GRID)), dim3(256), 0, sm, c, ep, st, ns, TJ_U8(op->b_due), TJ_U8(op->b_clr),
                       TJ_U32(op->b_keep), TJ_U32(op->b_pscan), op->ctr);
  }
  if ((rc = read_ctr(op))) return rc;
  const int64_t npad = (int64_t)op->hctr->n_pad_timer, nrm = (int64_t)op->hctr->n_rm_wm;
  const uint64_t fired[2] = {op->hctr->fired[0], op->hctr->fired[1]};
  // (the reference has no bound on a timer's output; max_pairs guards a push's pairs)
  if ((rc = grow_out(op, op->n_out + npad))) return rc;
  if (npad) {
    if ((rc = excl_scan<uint32_t>(op, TJ_U32(op->b_pscan), TJ_U32(op->b_spos), ns))) return rc;
    hipLaunchKernelGGL(k_tj_pad_store, dim3(gs), dim3(256), 0, sm, op->map, st, ns, TJ_U32(op->b_pscan),
                       TJ_U32(op->b_spos), op->out, op->n_out, (int64_t)0, true);
  }
  if (nrm) {
    if ((rc = excl_scan<uint32_t>(op, TJ_U32(op->b_keep), TJ_U32(op->b_kpos), ns))) return rc;
    hipLaunchKernelGGL(k_tj_compact, dim3(gs), dim3(256), 0, sm, st, ns, TJ_U32(op->b_keep), TJ_U32(op->b_kpos),
                       op->store[op->cur ^ 1]);
    op->cur ^= 1;
    op->n_store = ns - nrm;
  }
  hipLaunchKernelGGL(k_tj_wm_timers, dim3(gg), dim3(256), 0, sm, op->map, ng, TJ_U8(op->b_due), TJ_I64(op->b_tnew), op->ctr);
  if ((rc = read_ctr(op))) {
    op->ready = false;
    return rc;
  }
  op->next_due = op->hctr->next_due;
  for (int s = 0; s < 2; s++)
    if (fired[s]) op->X[s] = ep.E[s];
  op->n_out += npad;
  op->pad_timer += npad;
  append_segment(op, call, npad);
  if (n_rows) *n_rows = npad;
  return FW_OK;
}

}  // namespace

extern "C" {

int fw_tjoin_create(const fw_tjoin_config* cfg, fw_tjoin** out) {
  if (!cfg || !out) return FW_ERR_ARG;
  *out = nullptr;
  fw_tjoin* op = new fw_tjoin();
  op->cfg = *cfg;
  op->device = cfg->device;
  const fw_tjoin_config& c = *cfg;
  auto fail = [&](int code, const char* msg) {  // as fw_create: the handle carries the message; destroy it
    op->err = msg;
    *out = op;
    return code;
  };
  const int64_t B = int64_t(1) << 60;
  if (c.join_type < FW_TJOIN_INNER || c.join_type > FW_TJOIN_FULL)
    return fail(FW_ERR_ARG, "join_type must be FW_TJOIN_INNER, _LEFT, _RIGHT or _FULL");
  if (c.lower <= -B || c.lower >= B || c.upper <= -B || c.upper >= B)
    return fail(FW_ERR_ARG, "lower and upper must be inside (-2^60, 2^60)");
  if (c.lower > c.upper)
    return fail(FW_ERR_ARG, "lower > upper: a negative window size joins nothing and is planned without a join operator");
  if (c.allowed_lateness < 0) return fail(FW_ERR_ARG, "The allowed lateness must be non-negative.");
  if (c.allowed_lateness >= B) return fail(FW_ERR_ARG, "allowed_lateness must be below 2^60");
  if (c.max_pairs < 0) return fail(FW_ERR_ARG, "max_pairs must be >= 0");
  if (c.key_kind != FW_KEY_LONG && c.key_kind != FW_KEY_INT && c.key_kind != FW_KEY_HASHED)
    return fail(FW_ERR_ARG, "key_kind must be FW_KEY_LONG, FW_KEY_INT or FW_KEY_HASHED");
  if (c.max_parallelism < 1 || c.max_parallelism > 32768 || c.key_group_start < 0 ||
      c.key_group_end < c.key_group_start || c.key_group_end >= c.max_parallelism)
    return fail(FW_ERR_ARG, "max_parallelism must be in [1, 32768] and the KeyGroupRange inside [0, max_parallelism)");
  if (c.expected_keys < 0 || c.max_batch < 0) return fail(FW_ERR_ARG, "expected_keys and max_batch must be >= 0");
  TCfg& d = op->c;
  d.type = c.join_type;
  d.key_kind = c.key_kind;
  d.max_par = c.max_parallelism;
  d.kg0 = c.key_group_start;
  d.nkg = c.key_group_end - c.key_group_start + 1;
  d.rel[0] = -c.lower;
  d.rel[1] = c.upper;
  d.M = (d.rel[0] + d.rel[1]) / 2;
  d.L = c.allowed_lateness;
  op->max_rows = c.max_pairs > 0 ? c.max_pairs : (int64_t(1) << 30);
  *out = op;
  // ---- the GPU from here on
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || c.device < 0 || c.device >= ndev) {
    (void)hipGetLastError();
    return set_err(op, FW_ERR_HIP, "device %d is not available (%d devices)", c.device, ndev);
  }
  TB_HIP(op, hipSetDevice(c.device));
  TB_HIP(op, hipStreamCreateWithFlags(&op->stream, hipStreamNonBlocking));
  TB_HIP(op, hipMalloc(&op->ctr, sizeof(TCtr)));
  TB_HIP(op, hipHostMalloc(&op->hctr, sizeof(TCtr)));
  memset(op->hctr, 0, sizeof(TCtr));
  op->hctr->next_due = LMAX;
  op->hctr->first[0] = op->hctr->first[1] = LMAX;
  int rc;
  if ((rc = write_ctr(op))) return rc;
  const int64_t mb = c.max_batch > 0 ? c.max_batch : (int64_t(1) << 16);
  if ((rc = grow_map(op, std::max<int64_t>(c.expected_keys, 1024)))) return rc;
  if ((rc = grow_store(op, mb))) return rc;
  if ((rc = grow_run(op, mb))) return rc;
  op->ready = true;
  return FW_OK;
}

void fw_tjoin_destroy(fw_tjoin* op) {
  if (!op) return;
  if (op->stream) {
    (void)hipSetDevice(op->device);
    (void)hipStreamSynchronize(op->stream);
    free_map(op->map, slot_cols);
    for (TRows* r : {&op->store[0], &op->store[1], &op->run}) cols_free(row_cols(*r));
    cols_free(out_cols(op->out));
    (void)hipFree(op->ctr);
    (void)hipHostFree(op->hctr);
    (void)hipStreamDestroy(op->stream);
  }
  delete op;
}

const char* fw_tjoin_last_error(const fw_tjoin* op) { return op ? op->err.c_str() : "null handle"; }

int fw_tjoin_push_batch_device(fw_tjoin* op, const uint8_t* side, const int64_t* key, const int64_t* rowtime,
                               const int64_t* val, const int32_t* key_hash, int64_t n) {
  int rc;
  if ((rc = enter_push(op, !side || !key || !rowtime, key_hash, n)) || (rc = on_device(op))) return rc;
  return do_push(op, side, key, rowtime, val, key_hash, n);
}

int fw_tjoin_push_batch(fw_tjoin* op, const uint8_t* side, const int64_t* key, const int64_t* rowtime,
                        const int64_t* val, const int32_t* key_hash, int64_t n) {
  int rc;
  if ((rc = enter_push(op, !side || !key || !rowtime, key_hash, n))) return rc;
  if (n == 0) return FW_OK;
  if ((rc = on_device(op))) return rc;
  const size_t sz[5] = {(size_t)n, (size_t)n * 8, (size_t)n * 8, (size_t)n * 8, (size_t)n * 4};
  const void* src[5] = {side, key, rowtime, val, key_hash};
  for (int q = 0; q < 5; q++) {
    if (!src[q]) continue;
    if ((rc = ensure(op, op->b_stage[q], sz[q]))) return rc;
    TB_HIP(op, hipMemcpyAsync(op->b_stage[q].p, src[q], sz[q], hipMemcpyHostToDevice, op->stream));
  }
  // the staging copies run ahead of do_push's kernels on the same stream; its one read settles them too
  rc = do_push(op, (const uint8_t*)op->b_stage[0].p, (const int64_t*)op->b_stage[1].p, (const int64_t*)op->b_stage[2].p,
               val ? (const int64_t*)op->b_stage[3].p : nullptr, key_hash ? (const int32_t*)op->b_stage[4].p : nullptr, n);
  if (rc) (void)hipStreamSynchronize(op->stream);  // (a refusal before the read: the caller's columns are free again)
  return rc;
}

int fw_tjoin_advance_watermark(fw_tjoin* op, int64_t wm, int64_t* n_rows, int64_t* forwarded_wm) {
  int rc;
  if ((rc = enter(op))) return rc;
  if (wm < op->wm) return set_err(op, FW_ERR_ARG, "watermark %lld is lower than the current %lld", (long long)wm, (long long)op->wm);
  if ((rc = on_device(op)) || (rc = do_watermark(op, wm, n_rows))) return rc;
  // getMaxOutputDelay; the subtraction wraps as the reference's does
  if (forwarded_wm)
    *forwarded_wm = (int64_t)((uint64_t)wm - (uint64_t)(std::max(op->c.rel[0], op->c.rel[1]) + op->c.L));
  return FW_OK;
}

int fw_tjoin_drain(fw_tjoin* op, const fw_tjoin_rows* dst, int64_t* epoch, int64_t cap, int64_t* n) {
  int rc;
  if ((rc = enter(op, !dst || !n || cap < 0)) || (rc = on_device(op))) return rc;
  const TOut& o = op->out;
  return drain_pending(op, {{dst->key, o.key, 8}, {dst->left_ord, o.lord, 8}, {dst->right_ord, o.rord, 8},
                            {dst->left_rowtime, o.lts, 8}, {dst->right_rowtime, o.rts, 8}, {dst->left_val, o.lval, 8},
                            {dst->right_val, o.rval, 8}, {dst->cause_ord, o.cause, 8}, {dst->timer_ts, o.tts, 8}},
                       epoch, cap, n);
}

int fw_tjoin_rows_device(fw_tjoin* op, fw_tjoin_rows* rows, int64_t* n) {
  int rc;
  if ((rc = enter(op, !rows || !n)) || (rc = on_device(op)) || (rc = settle(op))) return rc;
  rows->key = op->out.key;
  rows->left_ord = op->out.lord;
  rows->right_ord = op->out.rord;
  rows->left_rowtime = op->out.lts;
  rows->right_rowtime = op->out.rts;
  rows->left_val = op->out.lval;
  rows->right_val = op->out.rval;
  rows->cause_ord = op->out.cause;
  rows->timer_ts = op->out.tts;
  *n = op->n_out;
  return FW_OK;
}

int fw_tjoin_clear_pending(fw_tjoin* op) {
  if (!op) return FW_ERR_ARG;
  clear_pending(op);
  return FW_OK;
}

int fw_tjoin_get_stats(fw_tjoin* op, fw_tjoin_stats* out) {
  if (!op || !out) return op ? set_err(op, FW_ERR_ARG, "null argument") : FW_ERR_ARG;
  memset(out, 0, sizeof *out);
  if (op->ready) {
    int rc;
    if ((rc = on_device(op)) || (rc = read_ctr(op))) return rc;
    out->timers_set = (int64_t)op->hctr->timers_set;
    out->active_timers = op->hctr->active_timers;
  }
  out->rows_in = op->rows_in;
  out->cached_rows = op->cached;
  out->rows_not_cached = op->not_cached;
  out->pairs = op->pairs;
  out->padded_at_arrival = op->pad_arr;
  out->padded_at_scan = op->pad_scan;
  out->padded_at_timer = op->pad_timer;
  out->pairs_with_expired_rows = op->exp_pairs;
  out->gate_skips = op->gate_skips;
  out->store_rows = op->n_store;
  out->current_watermark = op->wm;
  out->pending_output_rows = op->n_out;
  return FW_OK;
}

int fw_tjoin_snapshot_key_group(fw_tjoin* op, int32_t kg, const fw_tjoin_state* dst, int64_t cap_keys, int64_t cap_rows,
                                int64_t* n_keys, int64_t* n_rows) {
  int rc;
  if ((rc = enter_key_group(op, !n_keys || !n_rows, "null argument", kg)) || (rc = on_device(op)) || (rc = settle(op)))
    return rc;
  *n_keys = *n_rows = 0;
  const int64_t nsl = op->nslots, ns = op->n_store;
  if (nsl == 0) return FW_OK;
  // a checkpoint is not the hot path: the slots' columns and the store's group column cross, the host picks the key
  // group's keys (those with a timer set; a cache with rows always has its timer) and their rows
  std::vector<int64_t> skey(nsl), tmr(2 * nsl);
  std::vector<int32_t> skg(nsl);
  TB_HIP(op, hipMemcpy(skey.data(), op->map.skey, nsl * 8, hipMemcpyDeviceToHost));
  TB_HIP(op, hipMemcpy(skg.data(), op->map.skg, nsl * 4, hipMemcpyDeviceToHost));
  TB_HIP(op, hipMemcpy(tmr.data(), op->map.tmr, nsl * 16, hipMemcpyDeviceToHost));
  const TRows& st = op->store[op->cur];
  std::vector<uint32_t> g(ns);
  if (ns) TB_HIP(op, hipMemcpy(g.data(), st.g, ns * 4, hipMemcpyDeviceToHost));
  std::vector<int64_t> idx(nsl, -1), cnt;
  int64_t nk = 0, nr = 0;
  for (int64_t s = 0; s < nsl; s++)
    if (skg[s] == kg && (tmr[2 * s] | tmr[2 * s + 1]) != 0) idx[s] = nk++;
  cnt.assign(nk, 0);
  for (int64_t r = 0; r < ns; r++) {
    const int64_t i = idx[g[r] >> 1];
    if (i >= 0) {
      cnt[i]++;
      nr++;
    }
  }
  *n_keys = nk;
  *n_rows = nr;
  if (!dst || cap_keys < nk || cap_rows < nr || nk == 0) return FW_OK;
  std::vector<int64_t> ts(ns), ord(ns), val(ns);
  std::vector<uint8_t> em(ns);
  if (ns) {
    TB_HIP(op, hipMemcpy(ts.data(), st.ts, ns * 8, hipMemcpyDeviceToHost));
    TB_HIP(op, hipMemcpy(ord.data(), st.ord, ns * 8, hipMemcpyDeviceToHost));
    TB_HIP(op, hipMemcpy(val.data(), st.val, ns * 8, hipMemcpyDeviceToHost));
    TB_HIP(op, hipMemcpy(em.data(), st.emit, ns, hipMemcpyDeviceToHost));
  }
  std::vector<int64_t> fill(nk, 0);
  for (int64_t i = 1; i < nk; i++) fill[i] = fill[i - 1] + cnt[i - 1];
  for (int64_t s = 0; s < nsl; s++) {
    const int64_t i = idx[s];
    if (i < 0) continue;
    dst->key[i] = skey[s];
    dst->left_timer[i] = tmr[2 * s + 1];
    dst->right_timer[i] = tmr[2 * s];
    dst->n_rows[i] = cnt[i];
  }
  for (int64_t r = 0; r < ns; r++) {  // a key's rows: the left cache's, then the right's, each in (row time, ordinal) order
    const int64_t i = idx[g[r] >> 1];
    if (i < 0) continue;
    const int64_t d = fill[i]++;
    dst->side[d] = (uint8_t)(g[r] & 1u);
    dst->rowtime[d] = ts[r];
    dst->ordinal[d] = ord[r];
    dst->val[d] = val[r];
    dst->emitted[d] = em[r];
  }
  return FW_OK;
}

int fw_tjoin_restore_key_group(fw_tjoin* op, int32_t kg, const fw_tjoin_state* src, int64_t n_keys, int64_t n_rows) {
  int rc;
  if ((rc = enter_key_group(op, n_keys < 0 || n_rows < 0, "bad argument", kg))) return rc;
  if (n_keys == 0) return n_rows == 0 ? FW_OK : set_err(op, FW_ERR_ARG, "rows without keys");
  if (!src || !src->key || !src->left_timer || !src->right_timer || !src->n_rows ||
      (n_rows > 0 && (!src->side || !src->rowtime || !src->ordinal || !src->val || !src->emitted)))
    return set_err(op, FW_ERR_ARG, "null column");
  if ((rc = on_device(op)) || (rc = settle(op))) return rc;
  const TCfg& c = op->c;
  rc = check_restored_keys(op, c, kg, src->key, src->n_rows, n_keys, n_rows, [&](int64_t i) {
    return src->left_timer[i] < 0 || src->right_timer[i] < 0 ? set_err(op, FW_ERR_ARG, "negative timer") : FW_OK;
  });
  if (rc) return rc;
  int64_t max_ord = -1;
  for (int64_t r = 0; r < n_rows; r++) {
    if (src->side[r] > 1) return set_err(op, FW_ERR_ARG, "a restored row has a side outside {0, 1}");
    if (src->rowtime[r] < 0 || src->rowtime[r] >= TJ_TS_END)
      return set_err(op, FW_ERR_TIME_RANGE, "a restored row has a row time outside [0, 2^62)");
    max_ord = std::max(max_ord, src->ordinal[r]);
  }
  // a cache that holds rows has its timer set (the first cached row registers it; only the timer clears it): rows
  // without one would never be cleaned, and a snapshot, which picks the keys with a timer, would drop them
  for (int64_t i = 0, r = 0; i < n_keys; i++)
    for (int64_t q = 0; q < src->n_rows[i]; q++, r++)
      if ((src->side[r] == 0 ? src->right_timer[i] : src->left_timer[i]) == 0)
        return set_err(op, FW_ERR_ARG, "key %lld has %s cache rows but its %s is 0", (long long)src->key[i],
                       src->side[r] == 0 ? "left" : "right", src->side[r] == 0 ? "right_timer" : "left_timer");
  {
    std::unordered_set<int64_t> seen;
    if ((rc = check_restored_unique(op, src->key, n_keys, seen))) return rc;
    const int64_t nsl = op->nslots;
    std::vector<int64_t> skey(nsl), tmr(2 * nsl);
    if (nsl) {
      TB_HIP(op, hipMemcpy(skey.data(), op->map.skey, nsl * 8, hipMemcpyDeviceToHost));
      TB_HIP(op, hipMemcpy(tmr.data(), op->map.tmr, nsl * 16, hipMemcpyDeviceToHost));
    }
    for (int64_t s = 0; s < nsl; s++)
      if ((tmr[2 * s] | tmr[2 * s + 1]) != 0 && seen.count(skey[s]))
        return set_err(op, FW_ERR_STATE, "key %lld already has state in the handle", (long long)skey[s]);
  }
  if ((rc = grow_map(op, op->nslots + n_keys))) return rc;
  if ((rc = grow_store(op, op->n_store + n_rows))) return rc;
  if ((rc = grow_run(op, std::max<int64_t>(n_rows, 1)))) return rc;
  // rows in (row time, ordinal) order, each with its key; the device sorts them by group (stable)
  std::vector<int64_t> order(n_rows), hk(n_rows), ht(n_rows), ho(n_rows), hv(n_rows);
  std::vector<uint8_t> hs(n_rows), he(n_rows);
  {
    std::vector<int64_t> rkey(n_rows);
    int64_t r = 0;
    for (int64_t i = 0; i < n_keys; i++)
      for (int64_t q = 0; q < src->n_rows[i]; q++, r++) rkey[r] = src->key[i];
    std::iota(order.begin(), order.end(), int64_t(0));
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
      return src->rowtime[a] != src->rowtime[b] ? src->rowtime[a] < src->rowtime[b] : src->ordinal[a] < src->ordinal[b];
    });
    for (int64_t d = 0; d < n_rows; d++) {
      const int64_t q = order[d];
      hk[d] = rkey[q];
      ht[d] = src->rowtime[q];
      ho[d] = src->ordinal[q];
      hv[d] = src->val[q];
      hs[d] = src->side[q];
      he[d] = src->emitted[q] ? 1 : 0;
    }
  }
  Buf bk, bl, br, rk, rt, ro, rv, rs, re;
  auto up = [&](Buf& b, const void* p, size_t bytes) -> int {
    if (bytes == 0) return FW_OK;
    int e = ensure(op, b, bytes);
    if (e) return e;
    if (hipMemcpy(b.p, p, bytes, hipMemcpyHostToDevice) != hipSuccess) return set_err(op, FW_ERR_HIP, "hipMemcpy failed");
    return FW_OK;
  };
  rc = up(bk, src->key, n_keys * 8);
  if (!rc) rc = up(bl, src->left_timer, n_keys * 8);
  if (!rc) rc = up(br, src->right_timer, n_keys * 8);
  if (!rc) rc = up(rk, hk.data(), n_rows * 8);
  if (!rc) rc = up(rt, ht.data(), n_rows * 8);
  if (!rc) rc = up(ro, ho.data(), n_rows * 8);
  if (!rc) rc = up(rv, hv.data(), n_rows * 8);
  if (!rc) rc = up(rs, hs.data(), n_rows);
  if (!rc) rc = up(re, he.data(), n_rows);
  const int64_t ns = op->n_store;
  const size_t S = (size_t)std::max<int64_t>(ns, 1), R = (size_t)std::max<int64_t>(n_rows, 1);
  if (!rc) rc = ensure(op, op->b_keep, S * 4);
  if (!rc) rc = ensure(op, op->b_kpos, S * 4);
  if (!rc) rc = ensure(op, op->b_smark, S);
  if (!rc) rc = ensure(op, op->b_k2[0], R * 4);
  if (!rc) rc = ensure(op, op->b_k2[1], R * 4);
  if (!rc) rc = ensure(op, op->b_v1[0], R * 4);
  if (!rc) rc = ensure(op, op->b_v1[1], R * 4);
  if (!rc) {
    hipStream_t sm = op->stream;
    hipLaunchKernelGGL(k_tj_restore_keys, dim3(grid_of(n_keys)), dim3(256), 0, sm, c, op->map, op->ctr, kg,
                       (const int64_t*)bk.p, (const int64_t*)bl.p, (const int64_t*)br.p, n_keys);
    if (n_rows) {
      hipLaunchKernelGGL(k_tj_restore_groups, dim3(grid_of(n_rows)), dim3(256), 0, sm, op->map, (const int64_t*)rk.p,
                         (const uint8_t*)rs.p, n_rows, TJ_U32(op->b_k2[0]), TJ_U32(op->b_v1[0]));
      rc = sort_pairs<uint32_t>(op, TJ_U32(op->b_k2[0]), TJ_U32(op->b_k2[1]), TJ_U32(op->b_v1[0]), TJ_U32(op->b_v1[1]),
                                n_rows, group_bits(op));
      if (!rc) {
        hipLaunchKernelGGL(k_tj_restore_run, dim3(grid_of(n_rows)), dim3(256), 0, sm, TJ_U32(op->b_k2[1]),
                           TJ_U32(op->b_v1[1]), (const int64_t*)rt.p, (const int64_t*)ro.p, (const int64_t*)rv.p,
                           (const uint8_t*)re.p, n_rows, op->run);
        if (ns) hipLaunchKernelGGL(k_tj_iota, dim3(grid_of(ns)), dim3(256), 0, sm, TJ_U32(op->b_keep), TJ_U32(op->b_kpos), ns);
        if (hipMemsetAsync(op->b_smark.p, 0, S, sm) != hipSuccess) rc = set_err(op, FW_ERR_HIP, "hipMemsetAsync failed");
        if (!rc) merge_run(op, ns, n_rows);
      }
    }
    if (!rc) rc = read_ctr(op);
    if (rc) op->ready = false;
  }
  if (rc) return rc;
  op->nslots = op->hctr->nslots;
  op->next_due = op->hctr->next_due;
  op->ord_base = std::max(op->ord_base, max_ord + 1);
  return FW_OK;
}

}  // extern "C"
