// fw_over.hip — Table API OVER windows on row time (flink_window.h "fw_over_").
//
// The four ProcessFunctions of flink-table's runtime/aggregate/ (RowTimeBoundedRowsOver, RowTimeBoundedRangeOver,
// RowTimeUnboundedRowsOver, RowTimeUnboundedRangeOver) walk one key's rows in (row time, arrival) order and keep a
// running accumulator that they retract the rows leaving the frame from.  Here a watermark evaluates every frame at
// once:
//   push:      find or claim the key's slot, test the row (against the key's lastTriggeringTs or the watermark),
//              append kept rows to the row store (columns in HBM, arrival order)
//   watermark: mark the keys that have a row to fire -> split the store into the touched keys' rows <= wm and the
//              rest (stable) -> stable sort by (key, row time): a key's run in (row time, arrival) order -> frame
//              bounds per row (galloping searches; the bounds are monotone in a run) -> per column a segmented
//              inclusive scan of {non-null count, 128-bit sum | f64 sum} in tiles of OV_TILE rows with carried tile
//              aggregates -> per MIN / MAX a sparse table of spans 2 .. 64 built in LDS per tile plus a sparse table
//              over the 64-row blocks' minima -> one thread per firing row: its aggregates from prefix differences
//              and range minima, seeded by the key's accumulator (unbounded kinds) -> the keys' new state, the rows
//              some later frame can still reach back into the store.
// No kernel walks a key's rows: runs, peer groups and frames cross tiles and workgroups freely.
#include <unordered_map>

#include "fw_table.h"

namespace {

constexpr int OV_THREADS = 512, OV_ITEMS = 8, OV_TILE = OV_THREADS * OV_ITEMS;  // rows per scan workgroup
constexpr int OV_BLOCK = 64, OV_LEVELS = 6;  // range minima: spans 2^1 .. 2^6 per row, then one table over 64-row blocks
constexpr int OV_RT = 2048;                  // rows per sparse-table workgroup (+ OV_BLOCK halo in LDS)
constexpr uint64_t SIGN = 0x8000000000000000ull;

struct OCfg {
  int32_t kind, key_kind, max_par, kg0, nkg, nc, ns;
  int32_t ctype[8];
  int32_t agg[16];
  int64_t prec;
};
__host__ __device__ inline bool ov_bounded(const OCfg& c) { return c.kind <= FW_OVER_BOUNDED_RANGE; }
__host__ __device__ inline bool ov_rows(const OCfg& c) {
  return c.kind == FW_OVER_BOUNDED_ROWS || c.kind == FW_OVER_UNBOUNDED_ROWS;
}
__host__ __device__ inline int ov_accw(const OCfg& c) { return FW_OVER_ACC_WORDS(c.nc); }

struct OCtr {
  unsigned long long kept, late, no_ts, kg_err, map_full;
  long long next_due;  // the earliest pending row time (LMAX: none): a watermark below it has nothing to do
  long long due_rest;  // the same over the rows a watermark leaves in the store
  int32_t nslots;
  int32_t pad;
};

struct OMap : KeyMap {  // per key slot, besides the key and its key group
  int64_t* slast;    // lastTriggeringTs (bounded kinds), 0 = fresh
  int64_t* sacc;     // [slot * accw] the unbounded kinds' accumulator Row
  uint32_t* stouch;  // the watermark call that last found a row of the key to fire
};

struct ORowsD {  // the row store, or a watermark's gathered rows: columns of `cap` rows
  uint32_t* slot;
  int64_t *ts, *ord, *cols;
  uint8_t* nul;
  int64_t cap;
};

// Double.compare order as a signed integer order (every NaN the canonical one, Double.doubleToLongBits), and back
__host__ __device__ inline int64_t f64_unkey(int64_t k) { return k ^ (int64_t)((uint64_t)(k >> 63) >> 1); }
__host__ __device__ inline int64_t f64_key(int64_t b) {
  if ((b & 0x7ff0000000000000ll) == 0x7ff0000000000000ll && (b & 0x000fffffffffffffll)) b = 0x7ff8000000000000ll;
  return f64_unkey(b);
}
__device__ __forceinline__ bool f64_finite(int64_t b) { return (b & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }
__device__ __forceinline__ bool f64_nan(int64_t b) { return !f64_finite(b) && (b & 0x000fffffffffffffll); }
__host__ __device__ inline bool ov_float(int t) { return t == FW_VAL_F64 || t == FW_VAL_F32; }
__host__ __device__ inline int64_t ov_narrow(int t, int64_t v) {
  return t == FW_VAL_I32 ? (int64_t)(int32_t)v : t == FW_VAL_I16 ? (int64_t)(int16_t)v
       : t == FW_VAL_I8 ? (int64_t)(int8_t)v : v;
}

// ---------------------------------------------------------------- push
// refusals of a whole push: Long.MIN_VALUE row times, keys outside the KeyGroupRange
__global__ __launch_bounds__(256) void k_ov_check(OCfg c, const int64_t* __restrict__ key, const int64_t* __restrict__ ts,
                                                  const int32_t* __restrict__ kh, int64_t n, OCtr* ctr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool no_ts = false, bad_kg = false;
  if (i < n) {
    no_ts = ts[i] == LMIN;
    const int32_t kg = key_group(key_hash_of(c.key_kind, key[i], kh, i), c.max_par);
    bad_kg = kg < c.kg0 || kg >= c.kg0 + c.nkg;
  }
  const unsigned long long a = wave_count(no_ts), b = wave_count(bad_kg);
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&ctr->no_ts, a);
    if (b) atomicAdd(&ctr->kg_err, b);
  }
}
// per row: its key's slot and whether it is kept.  A bounded kind's lastTriggeringTs is never negative (0 when fresh,
// then row times above it), so a row time <= 0 is dropped without claiming a slot and every claim keeps its row.
__global__ __launch_bounds__(256) void k_ov_slots(OCfg c, OMap m, int64_t wm, const int64_t* __restrict__ key,
                                                  const int64_t* __restrict__ ts, const int32_t* __restrict__ kh,
                                                  int64_t n, uint32_t* __restrict__ pslot, uint32_t* __restrict__ pkeep,
                                                  OCtr* ctr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool late = false, kept = false;
  int64_t t = LMAX;
  if (i < n) {
    t = ts[i];
    const int64_t k = key[i];
    int32_t slot = -1;
    if (ov_bounded(c) ? t > 0 : t > wm) {
      slot = keymap_claim(m, &ctr->nslots, &ctr->map_full, k, [&] { return key_group(key_hash_of(c.key_kind, k, kh, i), c.max_par); });
      kept = slot >= 0 && (!ov_bounded(c) || t > m.slast[slot]);
    }
    late = !kept;
    pslot[i] = (uint32_t)slot;
    pkeep[i] = kept ? 1u : 0u;
  }
  const unsigned long long a = wave_count(late && i < n), b = wave_count(kept);
  const int64_t mn = wave_min64(kept ? t : LMAX);
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&ctr->late, a);
    if (b) {
      atomicAdd(&ctr->kept, b);
      atomicMin(&ctr->next_due, (long long)mn);
    }
  }
}
__global__ __launch_bounds__(256) void k_ov_append(OCfg c, ORowsD st, int64_t base, const int64_t* __restrict__ ts,
                                                   const int64_t* __restrict__ cols, const uint8_t* __restrict__ nulls,
                                                   int64_t n, int64_t ord_base, const uint32_t* __restrict__ pslot,
                                                   const uint32_t* __restrict__ pkeep, const uint32_t* __restrict__ ppos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !pkeep[i]) return;
  const int64_t d = base + ppos[i];
  if (d >= st.cap) return;  // (the host sized the store for the whole push)
  st.slot[d] = pslot[i];
  st.ts[d] = ts[i];
  st.ord[d] = jadd(ord_base, i);
  st.nul[d] = nulls ? nulls[i] : (uint8_t)0;
  for (int j = 0; j < c.nc; j++) st.cols[(int64_t)j * st.cap + d] = cols[(int64_t)j * n + i];
}

// ---------------------------------------------------------------- watermark: gather
__global__ __launch_bounds__(256) void k_ov_mark(OMap m, ORowsD st, int64_t n, int64_t wm, uint32_t epoch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t t = st.ts[i];
  const uint32_t s = st.slot[i];
  if (t <= wm && t > m.slast[s]) m.stouch[s] = epoch;
}
__global__ __launch_bounds__(256) void k_ov_select(OCfg c, OMap m, ORowsD st, int64_t n, int64_t wm, uint32_t epoch,
                                                   uint32_t* __restrict__ sel) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sel[i] = (st.ts[i] <= wm && (!ov_bounded(c) || m.stouch[st.slot[i]] == epoch)) ? 1u : 0u;
}
// selected rows: sort key (row time) and store index; the others move, in order, to the other store buffer
__global__ __launch_bounds__(256) void k_ov_split(OCfg c, OMap m, int64_t wm, ORowsD st, ORowsD dst, int64_t n,
                                                  const uint32_t* __restrict__ sel,
                                                  const uint32_t* __restrict__ pos, uint64_t* __restrict__ sk,
                                                  uint32_t* __restrict__ sv, OCtr* ctr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t rest = LMAX;
  if (i < n) {
    const uint32_t p = pos[i];
    if (sel[i]) {
      sk[p] = (uint64_t)st.ts[i] ^ SIGN;
      sv[p] = (uint32_t)i;
    } else {
      const int64_t d = i - p;
      const int64_t t = st.ts[i];
      const uint32_t s = st.slot[i];
      // still pending (an untouched key's retained rows are not): the next watermark that has work to do
      if (!ov_bounded(c) || t > wm || t > m.slast[s]) rest = t;
      dst.slot[d] = s;
      dst.ts[d] = t;
      dst.ord[d] = st.ord[i];
      dst.nul[d] = st.nul[i];
      for (int j = 0; j < c.nc; j++) dst.cols[(int64_t)j * dst.cap + d] = st.cols[(int64_t)j * st.cap + i];
    }
  }
  rest = wave_min64(rest);
  if ((threadIdx.x & 63) == 0 && rest != LMAX) atomicMin(&ctr->due_rest, (long long)rest);
}
// the second sort key: the row's key itself, not its slot (slots are handed out in the order the claims of a push
// happen to land; the key's value gives every run of the same input the same row order, hence the same scan tree)
__global__ __launch_bounds__(256) void k_ov_slot_keys(OMap mp, ORowsD st, const uint32_t* __restrict__ sv, int64_t m,
                                                      uint64_t* __restrict__ k2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) k2[i] = (uint64_t)mp.skey[st.slot[sv[i]]] ^ SIGN;
}
__global__ __launch_bounds__(256) void k_ov_gather(OCfg c, ORowsD st, ORowsD g, const uint32_t* __restrict__ perm, int64_t m) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int64_t s = perm[i];
  g.slot[i] = st.slot[s];
  g.ts[i] = st.ts[s];
  g.ord[i] = st.ord[s];
  g.nul[i] = st.nul[s];
  for (int j = 0; j < c.nc; j++) g.cols[(int64_t)j * g.cap + i] = st.cols[(int64_t)j * st.cap + s];
}

// ---------------------------------------------------------------- watermark: frames
// smallest idx in [a, b] with pred(idx), pred monotone (false .. false true .. true) and pred(b) true: galloping down
// from b, so a short run costs O(log run)
template <class P>
__device__ __forceinline__ int64_t first_true_down(int64_t a, int64_t b, P pred) {
  int64_t hi = b, lo = a, step = 1;
  while (true) {
    if (hi - a < step) {
      lo = a;
      break;
    }
    const int64_t cand = hi - step;
    if (pred(cand)) {
      hi = cand;
      step <<= 1;
    } else {
      lo = cand + 1;
      break;
    }
  }
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (pred(mid)) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// largest idx in [a, b] with pred(idx), pred monotone (true .. true false .. false) and pred(a) true
template <class P>
__device__ __forceinline__ int64_t last_true_up(int64_t a, int64_t b, P pred) {
  int64_t lo = a, hi = b, step = 1;
  while (true) {
    if (b - lo < step) {
      hi = b;
      break;
    }
    const int64_t cand = lo + step;
    if (pred(cand)) {
      lo = cand;
      step <<= 1;
    } else {
      hi = cand - 1;
      break;
    }
  }
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (pred(mid)) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// per gathered row: its frame [lo, hi] in the sorted rows, whether it fires, whether some later frame can reach it
__global__ __launch_bounds__(256) void k_ov_frames(OCfg c, OMap mp, ORowsD g, int64_t m, uint32_t* __restrict__ flo,
                                                   uint32_t* __restrict__ fhi, uint32_t* __restrict__ fire,
                                                   uint32_t* __restrict__ keep, uint32_t* __restrict__ fseg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t s = g.slot[i];
  const int64_t t = g.ts[i];
  const int64_t seg0 = first_true_down(0, i, [&](int64_t x) { return g.slot[x] == s; });
  const int64_t seg1 = last_true_up(i, m - 1, [&](int64_t x) { return g.slot[x] == s; });
  int64_t lo = seg0, hi = i;
  if (!ov_rows(c)) hi = last_true_up(i, seg1, [&](int64_t x) { return g.ts[x] == t; });  // the row's peers
  bool kp = false, fr = true;
  if (ov_bounded(c)) {
    const uint64_t p = (uint64_t)c.prec;
    if (ov_rows(c)) {
      lo = i - seg0 > c.prec ? i - c.prec : seg0;
      kp = (uint64_t)(seg1 - i) <= p;
    } else {
      // rows of the run are ordered by row time: the distance to an earlier row is exact as an unsigned difference
      lo = first_true_down(seg0, i, [&](int64_t x) { return (uint64_t)t - (uint64_t)g.ts[x] <= p; });
      kp = (uint64_t)g.ts[seg1] - (uint64_t)t <= p;
    }
    fr = t > mp.slast[s];
  }
  flo[i] = (uint32_t)lo;
  fhi[i] = (uint32_t)hi;
  fire[i] = fr ? 1u : 0u;
  keep[i] = kp ? 1u : 0u;
  if (fseg) fseg[i] = (uint32_t)seg0;
}

// ---------------------------------------------------------------- watermark: segmented scans
// the scan's element: a column's non-null count and sum over the rows since the run's start ("f": a run starts in
// here).  Integral sums are 128-bit two's complement (lo, hi) and wrap; a Double sum is the f64 in lo, and hi counts
// the column's +Inf values (low 32 bits) and -Inf values (high 32 bits).
struct SAcc {
  unsigned long long nn, lo;
  long long hi;
  uint32_t f;
};
template <bool F64>
__device__ __forceinline__ void sacc_add(SAcc& a, const SAcc& b) {  // a = a + b (values only)
  a.nn += b.nn;
  if (F64) {
    a.lo = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a.lo) +
                                                    __longlong_as_double((long long)b.lo));
    a.hi = (long long)((unsigned long long)a.hi + (unsigned long long)b.hi);
  } else {
    const unsigned long long l = a.lo + b.lo;
    a.hi = (long long)((unsigned long long)a.hi + (unsigned long long)b.hi + (l < a.lo ? 1ull : 0ull));
    a.lo = l;
  }
}
// segmented combine, `a` the earlier element: b unless no run starts in b
template <bool F64>
__device__ __forceinline__ SAcc sacc_comb(const SAcc& a, const SAcc& b) {
  if (b.f) return b;
  SAcc r = a;
  sacc_add<F64>(r, b);
  return r;
}
__device__ __forceinline__ SAcc sacc_shfl_up(const SAcc& x, int d) {
  SAcc r;
  r.nn = __shfl_up(x.nn, d, 64);
  r.lo = __shfl_up(x.lo, d, 64);
  r.hi = __shfl_up(x.hi, d, 64);
  r.f = __shfl_up(x.f, d, 64);
  return r;
}
// inclusive segmented scan of one element per thread over the workgroup (OV_THREADS); lds: OV_THREADS / 64 elements
template <bool F64>
__device__ SAcc block_seg_scan(SAcc x, SAcc* lds) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const SAcc t = sacc_shfl_up(x, d);
    if (lane >= d) x = sacc_comb<F64>(t, x);
  }
  if (lane == 63) lds[w] = x;
  __syncthreads();
  if (w > 0) {
    SAcc p = lds[0];
    for (int q = 1; q < w; q++) p = sacc_comb<F64>(p, lds[q]);  // (at most 7 wave aggregates, in wave order)
    x = sacc_comb<F64>(p, x);
  }
  __syncthreads();
  return x;
}
// pass 1: each tile's own scan (P: the scanned rows, relative to the tile's start), its aggregate and its first run start
template <bool F64>
__global__ __launch_bounds__(OV_THREADS) void k_ov_scan_tile(ORowsD g, int j, int64_t m, unsigned long long* __restrict__ pnn,
                                                             unsigned long long* __restrict__ plo, long long* __restrict__ phi,
                                                             SAcc* __restrict__ tagg, uint32_t* __restrict__ thead) {
  __shared__ SAcc lds[OV_THREADS / 64];
  __shared__ uint32_t first;
  if (threadIdx.x == 0) first = 0xffffffffu;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * OV_TILE + (int64_t)threadIdx.x * OV_ITEMS;
  SAcc v[OV_ITEMS];
  SAcc run{0, 0, 0, 0};
  uint32_t myfirst = 0xffffffffu;
  uint32_t prev_slot = (i0 > 0 && i0 <= m) ? g.slot[i0 - 1] : 0u;
#pragma unroll
  for (int r = 0; r < OV_ITEMS; r++) {
    const int64_t i = i0 + r;
    SAcc e{0, 0, 0, 0};
    if (i < m) {
      const uint32_t s = g.slot[i];
      e.f = (i == 0 || s != prev_slot) ? 1u : 0u;
      prev_slot = s;
      if (!((g.nul[i] >> j) & 1)) {
        const int64_t x = g.cols[(int64_t)j * g.cap + i];
        e.nn = 1;
        e.lo = (unsigned long long)x;
        e.hi = x < 0 ? -1ll : 0ll;
        if (F64) {
          // SumWithRetractAggFunction.scala:43-60 starts from +0.0, so its sum is never -0.0: neither is an element
          const double d = __longlong_as_double(x);
          e.lo = (unsigned long long)__double_as_longlong(0.0 + d);
          e.hi = d == __builtin_inf() ? 1ll : d == -__builtin_inf() ? (1ll << 32) : 0ll;
        }
      }
      if (e.f && myfirst == 0xffffffffu) myfirst = (uint32_t)i;
    }
    if (e.f) {
      run = e;
    } else {
      const uint32_t f = run.f;
      sacc_add<F64>(run, e);
      run.f = f;
    }
    v[r] = run;
  }
  if (myfirst != 0xffffffffu) atomicMin(&first, myfirst);
  const SAcc inc = block_seg_scan<F64>(run, lds);
  SAcc pre = sacc_shfl_up(inc, 1);  // the previous thread's inclusive value = this thread's exclusive one
  if ((threadIdx.x & 63) == 0) {
    // the first lane of a wave takes the last lane of the wave before it
    pre = SAcc{0, 0, 0, 0};
  }
  __shared__ SAcc last_of_wave[OV_THREADS / 64];
  if ((threadIdx.x & 63) == 63) last_of_wave[threadIdx.x >> 6] = inc;
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && threadIdx.x > 0) pre = last_of_wave[(threadIdx.x >> 6) - 1];
  const bool has_pre = threadIdx.x > 0;
#pragma unroll
  for (int r = 0; r < OV_ITEMS; r++) {
    const int64_t i = i0 + r;
    if (i >= m) break;
    SAcc o = v[r];
    if (has_pre && !o.f) {
      SAcc p = pre;
      sacc_add<F64>(p, o);
      o = p;
    }
    pnn[i] = o.nn;
    plo[i] = o.lo;
    phi[i] = o.hi;
  }
  if (threadIdx.x == OV_THREADS - 1) tagg[blockIdx.x] = inc;
  if (threadIdx.x == 0) thead[blockIdx.x] = first;  // (read after the atomics: ordered by the barriers above)
}
// pass 2: the tiles' aggregates scanned (exclusive) by one workgroup: carry[t] = the running value entering tile t
template <bool F64>
__global__ __launch_bounds__(OV_THREADS) void k_ov_scan_carry(const SAcc* __restrict__ tagg, int64_t ntiles,
                                                              SAcc* __restrict__ carry) {
  __shared__ SAcc lds[OV_THREADS / 64];
  __shared__ SAcc sh_run;
  __shared__ SAcc incs[OV_THREADS];
  if (threadIdx.x == 0) sh_run = SAcc{0, 0, 0, 0};
  __syncthreads();
  for (int64_t b = 0; b < ntiles; b += OV_THREADS) {
    const int64_t t = b + threadIdx.x;
    SAcc x{0, 0, 0, 0};
    if (t < ntiles) x = tagg[t];
    const SAcc inc = block_seg_scan<F64>(x, lds);
    incs[threadIdx.x] = inc;
    __syncthreads();
    const SAcc run = sh_run;
    if (t < ntiles) {
      SAcc ex = run;
      if (threadIdx.x > 0) ex = sacc_comb<F64>(run, incs[threadIdx.x - 1]);
      ex.f = 0;
      carry[t] = ex;
    }
    __syncthreads();
    if (threadIdx.x == OV_THREADS - 1) sh_run = sacc_comb<F64>(run, inc);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- watermark: range minima
// a MIN / MAX instance's order keys: the value's key (MAX: its complement, so every instance is a minimum), LMAX = NULL
__global__ __launch_bounds__(256) void k_ov_rmq_base(ORowsD g, int j, int is_max, int is_f, int64_t m, int64_t* __restrict__ base) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  int64_t k = LMAX;
  if (!((g.nul[i] >> j) & 1)) {
    k = g.cols[(int64_t)j * g.cap + i];
    if (is_f) k = f64_key(k);
    if (is_max) k = ~k;
  }
  base[i] = k;
}
// spans 2, 4, .. 64 from every row: st[(l - 1) * cap + i] = min(base[i .. i + 2^l - 1]) (clipped at m), built level by
// level in LDS for OV_RT rows and their halo; level 6 at a block's first row is the block's minimum (bt level 0)
__global__ __launch_bounds__(256) void k_ov_rmq_build(const int64_t* __restrict__ base, int64_t m, int64_t cap,
                                                      int64_t* __restrict__ st, int64_t* __restrict__ bt0) {
  __shared__ int64_t buf[2][OV_RT + OV_BLOCK];
  const int64_t t0 = (int64_t)blockIdx.x * OV_RT;
  for (int x = threadIdx.x; x < OV_RT + OV_BLOCK; x += blockDim.x) buf[0][x] = t0 + x < m ? base[t0 + x] : LMAX;
  __syncthreads();
  int cur = 0;
  for (int l = 1; l <= OV_LEVELS; l++) {
    const int half = 1 << (l - 1);
    for (int x = threadIdx.x; x < OV_RT + OV_BLOCK; x += blockDim.x) {
      const int64_t a = buf[cur][x];
      const int64_t b = x + half < OV_RT + OV_BLOCK ? buf[cur][x + half] : LMAX;
      const int64_t v = b < a ? b : a;
      buf[cur ^ 1][x] = v;
      if (x < OV_RT && t0 + x < m) {
        st[(int64_t)(l - 1) * cap + t0 + x] = v;
        if (l == OV_LEVELS && (x & (OV_BLOCK - 1)) == 0) bt0[(t0 + x) / OV_BLOCK] = v;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}
__global__ __launch_bounds__(256) void k_ov_rmq_blocks(const int64_t* __restrict__ prev, int64_t* __restrict__ next,
                                                       int64_t nb, int64_t half) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  const int64_t a = prev[b];
  const int64_t o = b + half < nb ? prev[b + half] : LMAX;
  next[b] = o < a ? o : a;
}
struct ORmq {
  const int64_t *base, *st, *bt;
  int64_t cap, nbcap;
};
__device__ __forceinline__ int64_t rmq_short(const ORmq& r, int64_t lo, int64_t hi) {  // hi - lo + 1 <= 64
  const uint32_t len = (uint32_t)(hi - lo + 1);
  const int k = 31 - __clz(len);
  if (k == 0) return r.base[lo];
  const int64_t a = r.st[(int64_t)(k - 1) * r.cap + lo];
  const int64_t b = r.st[(int64_t)(k - 1) * r.cap + (hi + 1 - ((int64_t)1 << k))];
  return b < a ? b : a;
}
__device__ __forceinline__ int64_t rmq_query(const ORmq& r, int64_t lo, int64_t hi) {
  if (hi - lo < OV_BLOCK) return rmq_short(r, lo, hi);
  const int64_t bl = lo / OV_BLOCK, bh = hi / OV_BLOCK;  // different blocks
  int64_t v = rmq_short(r, lo, bl * OV_BLOCK + OV_BLOCK - 1);
  const int64_t w = rmq_short(r, bh * OV_BLOCK, hi);
  v = w < v ? w : v;
  const int64_t nb = bh - bl - 1;
  if (nb > 0) {
    const int k = 63 - __clzll((unsigned long long)nb);
    const int64_t a = r.bt[(int64_t)k * r.nbcap + bl + 1];
    const int64_t b = r.bt[(int64_t)k * r.nbcap + (bh - ((int64_t)1 << k))];
    v = a < v ? a : v;
    v = b < v ? b : v;
  }
  return v;
}

// ---------------------------------------------------------------- watermark: evaluation
struct OScan {  // per column: the tiles' scans and carries (null for a column no aggregate reads)
  const unsigned long long* pnn[8];
  const unsigned long long* plo[8];
  const long long* phi[8];
  const SAcc* carry[8];
  const uint32_t* thead;
  ORmq mn[8], mx[8];  // base == null: none
  // bounded kinds, per Double column with a SUM / AVG: the rows where the key's sum turns non-finite (flags and their
  // exclusive scan), and every row's run start (null: none)
  const uint32_t* bad[8];
  const uint32_t* bcnt[8];
  const uint32_t* fseg;
};
// the scanned value at row i: the tile's own scan plus, before the tile's first run start, the carry
__device__ __forceinline__ SAcc scan_at(const OScan& sc, int j, bool f64, int64_t i) {
  SAcc a{sc.pnn[j][i], sc.plo[j][i], sc.phi[j][i], 0};
  const int64_t t = i / OV_TILE;
  if ((uint32_t)i < sc.thead[t]) {
    SAcc c = sc.carry[j][t];
    if (f64) sacc_add<true>(c, a); else sacc_add<false>(c, a);
    a = c;
  }
  return a;
}
// column j over the rows [lo, hi] of one run: the prefix difference (integral: exact, wrapping; Double: the run's
// prefix at hi minus its prefix before lo)
__device__ __forceinline__ SAcc frame_col(const OScan& sc, const ORowsD& g, int j, bool f64, int64_t lo, int64_t hi) {
  SAcc a = scan_at(sc, j, f64, hi);
  if (lo > 0 && g.slot[lo - 1] == g.slot[lo]) {
    const SAcc b = scan_at(sc, j, f64, lo - 1);
    a.nn -= b.nn;
    if (f64) {
      a.lo = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a.lo) -
                                                      __longlong_as_double((long long)b.lo));
      a.hi = (long long)((unsigned long long)a.hi - (unsigned long long)b.hi);
    } else {
      const unsigned long long l = a.lo - b.lo;
      a.hi = (long long)((unsigned long long)a.hi - (unsigned long long)b.hi - (a.lo < b.lo ? 1ull : 0ull));
      a.lo = l;
    }
  }
  return a;
}
// ---- bounded kinds, Double SUM / AVG: the sum that is not finite.  The reference keeps one accumulator per key, adds
// the rows entering the frame and subtracts the rows leaving it (SumWithRetractAggFunction.scala:43-60), so a sum that
// is NaN or infinite once is never finite again for the key: +Inf stays until a -Inf or a NaN is added or a +Inf is
// subtracted (NaN from then on), -Inf likewise.  Up to the first such row of a key a frame's prefix difference is the
// reference's value; from it on the value is that row's (or, across watermarks, the key's carried one: the sum word
// of the slot's accumulator, 0 while the last emitted sum was finite) unless one of those events lies between.
__device__ __forceinline__ int64_t* ov_carry(const OCfg& c, const OMap& mp, uint32_t slot, int j) {
  return mp.sacc + (int64_t)slot * ov_accw(c) + 2 + 5 * j;
}
// flags: a firing row whose frame's sum is not finite; the key's last fired row when the key carries such a sum
__global__ __launch_bounds__(256) void k_ov_nonfinite(OCfg c, OMap mp, OScan sc, ORowsD g, int j, int64_t m,
                                                      const uint32_t* __restrict__ flo, const uint32_t* __restrict__ fhi,
                                                      const uint32_t* __restrict__ fire, uint32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  bool b;
  if (fire[i]) b = !f64_finite((int64_t)frame_col(sc, g, j, true, flo[i], fhi[i]).lo);
  else b = i + 1 < m && fire[i + 1] && g.slot[i + 1] == g.slot[i] && !f64_finite(*ov_carry(c, mp, g.slot[i], j));
  bad[i] = b ? 1u : 0u;
}
// the sum of firing row i's frame, `sum` its prefix difference
__device__ int64_t ov_sticky_sum(const OCfg& c, const OMap& mp, const OScan& sc, const ORowsD& g, int j, int64_t i,
                                 const uint32_t* flo, const uint32_t* fhi, const uint32_t* fire, int64_t sum) {
  const uint32_t *bad = sc.bad[j], *cnt = sc.bcnt[j];
  const int64_t seg0 = sc.fseg[i];
  const uint32_t base = cnt[seg0];
  if (cnt[i] + bad[i] == base) return sum;  // finite so far
  const int64_t e = first_true_down(seg0, i, [&](int64_t x) { return cnt[x] + bad[x] != base; });
  if (e == i) return sum;                   // the first one
  const int64_t s0 = fire[e] ? (int64_t)frame_col(sc, g, j, true, flo[e], fhi[e]).lo : *ov_carry(c, mp, g.slot[e], j);
  if (f64_nan(s0)) return s0;
  // since row e: the infinities added (the rows behind e's frame end up to i's) and subtracted (the rows from e's
  // frame start to before i's), {+Inf, -Inf} counts packed as in the scan
  const SAcc ph = scan_at(sc, j, true, fhi[i]);
  const unsigned long long added = (unsigned long long)ph.hi - (unsigned long long)scan_at(sc, j, true, fhi[e]).hi;
  const int64_t li = flo[i], le = flo[e];
  const unsigned long long gone = (li > seg0 ? (unsigned long long)scan_at(sc, j, true, li - 1).hi : 0ull) -
                                  (le > seg0 ? (unsigned long long)scan_at(sc, j, true, le - 1).hi : 0ull);
  const bool pos = s0 > 0;  // (the bits of +Inf)
  const bool broken = f64_nan((int64_t)ph.lo) || (pos ? (added >> 32) != 0 || (uint32_t)gone != 0
                                                      : (uint32_t)added != 0 || (gone >> 32) != 0);
  return broken ? 0x7ff8000000000000ll : s0;
}

// |x| / d of a 128-bit two's-complement x (d >= 1) toward zero (BigInteger.divide, AvgAggFunction.scala:160-166)
__device__ int64_t ov_div128(unsigned long long lo, long long hi, unsigned long long d) {
  const bool neg = hi < 0;
  unsigned long long ul = lo, uh = (unsigned long long)hi;
  if (neg) {
    ul = ~ul + 1ull;
    uh = ~uh + (ul == 0ull ? 1ull : 0ull);
  }
  unsigned long long q = 0, r = uh % d;
  for (int b = 63; b >= 0; b--) {
    const bool top = (r >> 63) != 0;
    r = (r << 1) | ((ul >> b) & 1ull);
    if (top || r >= d) {
      r -= d;
      q |= 1ull << b;
    }
  }
  return neg ? (int64_t)(0ull - q) : (int64_t)q;
}
// the frame's column aggregate joined with the key's accumulator (unbounded kinds): words nn, lo, hi, mn, mx of sacc
struct OCol {
  SAcc s;
  int64_t mn, mx;  // order keys (valid when s.nn > 0)
};
__device__ OCol ov_col(const OCfg& c, const OScan& sc, const ORowsD& g, const int64_t* acc, int j, int64_t lo, int64_t hi,
                       bool want_mn, bool want_mx) {
  const bool f64 = ov_float(c.ctype[j]);
  OCol o;
  o.s = frame_col(sc, g, j, f64, lo, hi);
  o.mn = LMAX;
  o.mx = LMIN;
  if (o.s.nn) {
    if (want_mn && sc.mn[j].base) o.mn = rmq_query(sc.mn[j], lo, hi);
    if (want_mx && sc.mx[j].base) o.mx = ~rmq_query(sc.mx[j], lo, hi);
  }
  if (acc) {
    const int64_t* a = acc + 1 + 5 * j;
    if (a[0]) {
      SAcc seed{(unsigned long long)a[0], (unsigned long long)a[1], a[2], 0};
      const int64_t smn = f64 ? f64_key(a[3]) : a[3], smx = f64 ? f64_key(a[4]) : a[4];
      if (f64) sacc_add<true>(seed, o.s); else sacc_add<false>(seed, o.s);  // the accumulator first, then the frame
      o.mn = o.s.nn && o.mn < smn ? o.mn : smn;
      o.mx = o.s.nn && o.mx > smx ? o.mx : smx;
      o.s = seed;
    }
  }
  return o;
}
__global__ __launch_bounds__(256) void k_ov_eval(OCfg c, OMap mp, OScan sc, ORowsD g, int64_t m, const uint32_t* __restrict__ flo,
                                                 const uint32_t* __restrict__ fhi, const uint32_t* __restrict__ fire,
                                                 const uint32_t* __restrict__ opos, int64_t obase, int64_t ocap,
                                                 int64_t* __restrict__ okey, int64_t* __restrict__ ots,
                                                 int64_t* __restrict__ oord, int64_t* __restrict__ oval,
                                                 uint32_t* __restrict__ onul) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || !fire[i]) return;
  const int64_t d = obase + opos[i];
  if (d >= ocap) return;  // (sized from the exact count)
  const int64_t lo = flo[i], hi = fhi[i];
  const uint32_t slot = g.slot[i];
  const int64_t* acc = ov_bounded(c) ? nullptr : mp.sacc + (int64_t)slot * ov_accw(c);
  okey[d] = mp.skey[slot];
  ots[d] = g.ts[i];
  oord[d] = g.ord[i];
  uint32_t nm = 0;
  for (int q = 0; q < c.ns; q++) {
    const int fn = c.agg[q] >> 8, j = c.agg[q] & 0xff;
    int64_t v = 0;
    if (fn == FW_ROW_COUNT_STAR) {
      v = hi - lo + 1 + (acc ? acc[0] : 0);
    } else {
      const int t = c.ctype[j];
      OCol o = ov_col(c, sc, g, acc, j, lo, hi, fn == FW_ROW_MIN, fn == FW_ROW_MAX);
      if (sc.bad[j] && (fn == FW_ROW_SUM || fn == FW_ROW_AVG))
        o.s.lo = (unsigned long long)ov_sticky_sum(c, mp, sc, g, j, i, flo, fhi, fire, (int64_t)o.s.lo);
      if (fn == FW_ROW_COUNT) {
        v = (int64_t)o.s.nn;
      } else if (o.s.nn == 0) {
        nm |= 1u << q;
      } else if (fn == FW_ROW_SUM) {
        v = ov_float(t) ? (int64_t)o.s.lo : ov_narrow(t, (int64_t)o.s.lo);
      } else if (fn == FW_ROW_MIN) {
        v = ov_float(t) ? f64_unkey(o.mn) : o.mn;
      } else if (fn == FW_ROW_MAX) {
        v = ov_float(t) ? f64_unkey(o.mx) : o.mx;
      } else {  // FW_ROW_AVG
        if (ov_float(t)) v = __double_as_longlong(__longlong_as_double((long long)o.s.lo) / (double)o.s.nn);
        else if (t == FW_VAL_I64) v = ov_div128(o.s.lo, o.s.hi, o.s.nn);
        else v = ov_narrow(t, (int64_t)o.s.lo / (int64_t)o.s.nn);
      }
    }
    oval[d * c.ns + q] = v;
  }
  onul[d] = nm;
}
// the keys' new state, by the thread of each run's last row (one per key; the evaluation has read the old state)
__global__ __launch_bounds__(256) void k_ov_state(OCfg c, OMap mp, OScan sc, ORowsD g, int64_t m, const uint32_t* __restrict__ flo,
                                                  const uint32_t* __restrict__ fhi, const uint32_t* __restrict__ fire,
                                                  uint32_t used_cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || !fire[i]) return;
  const uint32_t slot = g.slot[i];
  if (i + 1 < m && g.slot[i + 1] == slot) return;
  if (ov_bounded(c)) {
    mp.slast[slot] = g.ts[i];
    for (int j = 0; j < c.nc; j++) {  // the last emitted Double sum, kept while it is not finite
      if (!sc.bad[j]) continue;
      const int64_t s = ov_sticky_sum(c, mp, sc, g, j, i, flo, fhi, fire, (int64_t)frame_col(sc, g, j, true, flo[i], fhi[i]).lo);
      *ov_carry(c, mp, slot, j) = f64_finite(s) ? 0 : s;
    }
    return;
  }
  int64_t* acc = mp.sacc + (int64_t)slot * ov_accw(c);
  const int64_t lo = flo[i];
  for (int j = 0; j < c.nc; j++) {
    if (!((used_cols >> j) & 1)) continue;
    const bool f64 = ov_float(c.ctype[j]);
    const OCol o = ov_col(c, sc, g, acc, j, lo, i, true, true);
    int64_t* a = acc + 1 + 5 * j;
    a[0] = (int64_t)o.s.nn;
    a[1] = (int64_t)o.s.lo;
    a[2] = f64 ? 0 : o.s.hi;  // (a Double's Inf counts are a run's own)
    a[3] = o.s.nn && sc.mn[j].base ? (f64 ? f64_unkey(o.mn) : o.mn) : 0;
    a[4] = o.s.nn && sc.mx[j].base ? (f64 ? f64_unkey(o.mx) : o.mx) : 0;
  }
  acc[0] = jadd(acc[0], i - lo + 1);
}
// the gathered rows some later frame can reach, back into the store behind the rows the split left there
__global__ __launch_bounds__(256) void k_ov_retain(OCfg c, ORowsD g, ORowsD dst, int64_t m, int64_t base,
                                                   const uint32_t* __restrict__ keep, const uint32_t* __restrict__ kpos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || !keep[i]) return;
  const int64_t d = base + kpos[i];
  if (d >= dst.cap) return;
  dst.slot[d] = g.slot[i];
  dst.ts[d] = g.ts[i];
  dst.ord[d] = g.ord[i];
  dst.nul[d] = g.nul[i];
  for (int j = 0; j < c.nc; j++) dst.cols[(int64_t)j * dst.cap + d] = g.cols[(int64_t)j * g.cap + i];
}
// total of a 0 / 1 flag array from its exclusive scan
__global__ void k_ov_total(const uint32_t* flag, const uint32_t* pos, int64_t n, unsigned long long* out) {
  *out = n > 0 ? (unsigned long long)pos[n - 1] + flag[n - 1] : 0ull;
}

// ---------------------------------------------------------------- snapshot
// the slots and the rows of key group kg, flagged (then scanned by the host's launches) and packed
__global__ __launch_bounds__(256) void k_ov_snap_flags(OMap m, ORowsD st, int64_t ns, int64_t n, int32_t kg,
                                                       uint32_t* __restrict__ fs, uint32_t* __restrict__ fr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ns) fs[i] = m.skg[i] == kg ? 1u : 0u;
  if (i < n) fr[i] = m.skg[st.slot[i]] == kg ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_ov_snap_pack(OCfg c, OMap m, ORowsD st, int64_t ns, int64_t n,
                                                      const uint32_t* __restrict__ fs, const uint32_t* __restrict__ ps,
                                                      const uint32_t* __restrict__ fr, const uint32_t* __restrict__ pr,
                                                      uint32_t* __restrict__ oss, int64_t* __restrict__ osw,
                                                      uint32_t* __restrict__ ors, int64_t* __restrict__ orw,
                                                      uint8_t* __restrict__ orn) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int w = ov_accw(c);
  if (i < ns && fs[i]) {
    const int64_t d = ps[i];
    oss[d] = (uint32_t)i;
    int64_t* o = osw + d * (2 + w);
    o[0] = m.skey[i];
    o[1] = m.slast[i];
    for (int q = 0; q < w; q++) o[2 + q] = m.sacc[i * w + q];
  }
  if (i < n && fr[i]) {
    const int64_t d = pr[i];
    ors[d] = st.slot[i];
    int64_t* o = orw + d * (2 + c.nc);
    o[0] = st.ts[i];
    o[1] = st.ord[i];
    for (int j = 0; j < c.nc; j++) o[2 + j] = st.cols[(int64_t)j * st.cap + i];
    orn[d] = st.nul[i];
  }
}

// ---------------------------------------------------------------- restore
__global__ __launch_bounds__(256) void k_ov_restore_keys(OCfg c, OMap m, OCtr* ctr, int32_t kg, const int64_t* __restrict__ key,
                                                         const int64_t* __restrict__ last, const int64_t* __restrict__ acc,
                                                         int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t slot = keymap_claim(m, &ctr->nslots, &ctr->map_full, key[i], [&] { return kg; });
  if (slot < 0) return;
  m.slast[slot] = ov_bounded(c) ? last[i] : 0;
  const int w = ov_accw(c);  // (a bounded key's words: zero but for a carried non-finite Double sum)
  for (int q = 0; q < w; q++) m.sacc[(int64_t)slot * w + q] = acc[i * w + q];
}
__global__ __launch_bounds__(256) void k_ov_restore_rows(OCfg c, OMap m, ORowsD st, int64_t base, const int64_t* __restrict__ key,
                                                         const int64_t* __restrict__ ts, const int64_t* __restrict__ ord,
                                                         const int64_t* __restrict__ cols, const uint8_t* __restrict__ nul,
                                                         int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t d = base + i;
  if (d >= st.cap) return;
  st.slot[d] = (uint32_t)keymap_find(m, key[i]);
  st.ts[d] = ts[i];
  st.ord[d] = ord[i];
  st.nul[d] = nul[i];
  for (int j = 0; j < c.nc; j++) st.cols[(int64_t)j * st.cap + d] = cols[i * c.nc + j];
}

struct OOut {  // the pending output rows: columns of the handle's `ocap` rows (val: ns words a row)
  int64_t *key, *ts, *ord, *val;
  uint32_t* nul;
};

}  // namespace

struct fw_over : TableHandle {  // (oseg's epochs: the watermark calls)
  fw_over_config cfg{};
  OCfg c{};
  OMap map{};
  OCtr* ctr = nullptr;       // device
  OCtr* hctr = nullptr;      // pinned host copy
  unsigned long long* tot = nullptr;  // device [2]
  ORowsD store[2]{};
  int cur = 0;
  int64_t n_store = 0, pending = 0;
  int64_t nslots = 0;
  int64_t wm = LMIN, next_due = LMAX, ord_base = 0;
  int64_t kept_total = 0, late_total = 0, fired_total = 0;
  uint32_t epoch = 0;        // watermark calls that did work (stouch's stamp)
  int64_t wm_calls = 0;
  OOut out{};
  uint32_t used_cols = 0, min_cols = 0, max_cols = 0;
  uint32_t fsum_cols = 0;    // bounded kinds: the Double columns with a SUM / AVG
  Buf b_fseg, b_bad[8], b_bcnt[8];
  Buf b_stage[5], b_pslot, b_pkeep, b_ppos, b_sel, b_pos, b_sk[2], b_sv[2], b_k2[2];
  Buf b_g[5], b_flo, b_fhi, b_fire, b_keep, b_opos, b_kpos, b_thead;
  Buf b_pnn[8], b_plo[8], b_phi[8], b_tagg[8], b_carry[8];
  Buf b_rbase[16], b_rst[16], b_rbt[16];
};

namespace {

// the column sets: the row store (cols: a column-major matrix, one plane per column), a key slot's state, the output
auto row_cols(const fw_over* op) {
  return [nc = op->c.nc](ORowsD& r) { return Cols{col(r.slot), col(r.ts), col(r.ord), col(r.cols, 8, nc), col(r.nul)}; };
}
auto slot_cols(const fw_over* op) {  // (besides the key map's own skey, skg)
  return [w = (size_t)8 * ov_accw(op->c)](OMap& m) { return Cols{col(m.slast, 8, 1, 0), col(m.sacc, w, 1, 0), col(m.stouch, 4, 1, 0)}; };
}
auto out_cols(const fw_over* op) {
  return [w = (size_t)8 * op->c.ns](OOut& o) { return Cols{col(o.key), col(o.ts), col(o.ord), col(o.val, w), col(o.nul)}; };
}

int grow_store(fw_over* op, int64_t need) {
  return grow_store(op, op->store, op->cur, op->n_store, need, row_cols(op));
}
int grow_map(fw_over* op, int64_t keys) {
  return grow_map(op, op->map, op->nslots, keys, 30, slot_cols(op));
}
int grow_out(fw_over* op, int64_t need) {
  return cols_grow(op, op->out, op->ocap, need, op->n_out, out_cols(op), "cannot allocate an output buffer of %lld rows");
}

template <bool F64>
void launch_scan(fw_over* op, const ORowsD& g, int j, int64_t m, int64_t ntiles) {
  hipLaunchKernelGGL(k_ov_scan_tile<F64>, dim3((unsigned)ntiles), dim3(OV_THREADS), 0, op->stream, g, j, m,
                     (unsigned long long*)op->b_pnn[j].p, (unsigned long long*)op->b_plo[j].p, (long long*)op->b_phi[j].p,
                     (SAcc*)op->b_tagg[j].p, (uint32_t*)op->b_thead.p);
  hipLaunchKernelGGL(k_ov_scan_carry<F64>, dim3(1), dim3(OV_THREADS), 0, op->stream, (const SAcc*)op->b_tagg[j].p, ntiles,
                     (SAcc*)op->b_carry[j].p);
}

int do_push(fw_over* op, const int64_t* key, const int64_t* ts, const int64_t* cols, const uint8_t* nulls,
            const int32_t* kh, int64_t n) {
  if (n == 0) return FW_OK;
  int rc;
  if ((rc = grow_store(op, op->n_store + n))) return rc;
  if ((rc = grow_map(op, op->nslots + n))) return rc;
  if ((rc = ensure(op, op->b_pslot, (size_t)n * 4)) || (rc = ensure(op, op->b_pkeep, (size_t)n * 4)) ||
      (rc = ensure(op, op->b_ppos, (size_t)n * 4)))
    return rc;
  hipLaunchKernelGGL(k_ov_check, dim3(grid_of(n)), dim3(256), 0, op->stream, op->c, key, ts, kh, n, op->ctr);
  if ((rc = read_ctr(op))) return rc;
  if (op->hctr->no_ts || op->hctr->kg_err) {
    const unsigned long long a = op->hctr->no_ts, b = op->hctr->kg_err;
    op->hctr->no_ts = op->hctr->kg_err = 0;
    if ((rc = write_ctr(op))) return rc;
    if (a)
      return set_err(op, FW_ERR_NO_TIMESTAMP, "%llu row(s) with a Long.MIN_VALUE row time; the push was refused", a);
    return set_err(op, FW_ERR_KEY_GROUP, "%llu row(s) outside KeyGroupRange [%d, %d]; the push was refused", b,
                   op->c.kg0, op->c.kg0 + op->c.nkg - 1);
  }
  uint32_t *pslot = (uint32_t*)op->b_pslot.p, *pkeep = (uint32_t*)op->b_pkeep.p, *ppos = (uint32_t*)op->b_ppos.p;
  hipLaunchKernelGGL(k_ov_slots, dim3(grid_of(n)), dim3(256), 0, op->stream, op->c, op->map, op->wm, key, ts, kh, n, pslot,
                     pkeep, op->ctr);
  if ((rc = excl_scan(op, pkeep, ppos, n))) return rc;
  hipLaunchKernelGGL(k_ov_append, dim3(grid_of(n)), dim3(256), 0, op->stream, op->c, op->store[op->cur], op->n_store, ts,
                     cols, nulls, n, op->ord_base, pslot, pkeep, ppos);
  if ((rc = read_ctr(op))) return rc;
  TB_HIP(op, hipGetLastError());
  if (op->hctr->map_full) return set_err(op, FW_ERR_STATE, "the key map overflowed");
  const int64_t kept = (int64_t)op->hctr->kept - op->kept_total;
  op->kept_total = (int64_t)op->hctr->kept;
  op->late_total = (int64_t)op->hctr->late;
  op->nslots = op->hctr->nslots;
  op->next_due = op->hctr->next_due;
  op->n_store += kept;
  op->pending += kept;
  op->ord_base += n;
  return FW_OK;
}

int do_watermark(fw_over* op, int64_t wm, int64_t* n_rows) {
  if (n_rows) *n_rows = 0;
  const int64_t call = op->wm_calls++;
  op->wm = wm;
  if (wm < op->next_due || op->n_store == 0) return FW_OK;  // nothing is due
  const OCfg& c = op->c;
  const int64_t n = op->n_store;
  int rc;
  const uint32_t epoch = ++op->epoch;
  ORowsD st = op->store[op->cur], other = op->store[op->cur ^ 1];
  if ((rc = ensure(op, op->b_sel, (size_t)n * 4)) || (rc = ensure(op, op->b_pos, (size_t)n * 4))) return rc;
  for (int h = 0; h < 2; h++)
    if ((rc = ensure(op, op->b_sk[h], (size_t)n * 8)) || (rc = ensure(op, op->b_sv[h], (size_t)n * 4)) ||
        (rc = ensure(op, op->b_k2[h], (size_t)n * 8)))
      return rc;
  uint32_t *sel = (uint32_t*)op->b_sel.p, *pos = (uint32_t*)op->b_pos.p;
  if (ov_bounded(c)) hipLaunchKernelGGL(k_ov_mark, dim3(grid_of(n)), dim3(256), 0, op->stream, op->map, st, n, wm, epoch);
  hipLaunchKernelGGL(k_ov_select, dim3(grid_of(n)), dim3(256), 0, op->stream, c, op->map, st, n, wm, epoch, sel);
  if ((rc = excl_scan(op, sel, pos, n))) return rc;
  hipLaunchKernelGGL(k_ov_total, dim3(1), dim3(1), 0, op->stream, sel, pos, n, op->tot);
  op->hctr->due_rest = LMAX;  // (hctr mirrors the device after the last read_ctr)
  TB_HIP(op, hipMemcpyAsync(&op->ctr->due_rest, &op->hctr->due_rest, 8, hipMemcpyHostToDevice, op->stream));
  hipLaunchKernelGGL(k_ov_split, dim3(grid_of(n)), dim3(256), 0, op->stream, c, op->map, wm, st, other, n, sel, pos,
                     (uint64_t*)op->b_sk[0].p, (uint32_t*)op->b_sv[0].p, op->ctr);
  unsigned long long htot[2] = {0, 0};
  TB_HIP(op, hipMemcpyAsync(htot, op->tot, 8, hipMemcpyDeviceToHost, op->stream));
  TB_HIP(op, hipStreamSynchronize(op->stream));
  const int64_t m = (int64_t)htot[0], rest = n - m;
  if (m == 0) {  // (next_due was stale: rows below it were all retained ones of untouched keys)
    op->cur ^= 1;
    if ((rc = read_ctr(op))) return rc;
    op->next_due = op->hctr->next_due = op->hctr->due_rest;
    return write_ctr(op);
  }
  // stable sort by row time, then by key: a key's run in (row time, arrival) order
  {
    uint64_t *sk0 = (uint64_t*)op->b_sk[0].p, *sk1 = (uint64_t*)op->b_sk[1].p;
    uint64_t *k20 = (uint64_t*)op->b_k2[0].p, *k21 = (uint64_t*)op->b_k2[1].p;
    uint32_t *sv0 = (uint32_t*)op->b_sv[0].p, *sv1 = (uint32_t*)op->b_sv[1].p;
    if ((rc = sort_pairs<uint64_t>(op, sk0, sk1, sv0, sv1, m, 64u))) return rc;
    hipLaunchKernelGGL(k_ov_slot_keys, dim3(grid_of(m)), dim3(256), 0, op->stream, op->map, st, (const uint32_t*)sv1, m, k20);
    if ((rc = sort_pairs<uint64_t>(op, k20, k21, sv1, sv0, m, 64u))) return rc;  // (sv0: the rows' final order)
    // the gathered rows
    const size_t sz[5] = {(size_t)m * 4, (size_t)m * 8, (size_t)m * 8, (size_t)m * 8 * c.nc, (size_t)m};
    for (int q = 0; q < 5; q++)
      if ((rc = ensure(op, op->b_g[q], sz[q]))) return rc;
    ORowsD g{(uint32_t*)op->b_g[0].p, (int64_t*)op->b_g[1].p, (int64_t*)op->b_g[2].p, (int64_t*)op->b_g[3].p,
             (uint8_t*)op->b_g[4].p, m};
    hipLaunchKernelGGL(k_ov_gather, dim3(grid_of(m)), dim3(256), 0, op->stream, c, st, g, (const uint32_t*)sv0, m);
  }
  ORowsD g{(uint32_t*)op->b_g[0].p, (int64_t*)op->b_g[1].p, (int64_t*)op->b_g[2].p, (int64_t*)op->b_g[3].p,
           (uint8_t*)op->b_g[4].p, m};
  if ((rc = ensure(op, op->b_flo, (size_t)m * 4)) || (rc = ensure(op, op->b_fhi, (size_t)m * 4)) ||
      (rc = ensure(op, op->b_fire, (size_t)m * 4)) || (rc = ensure(op, op->b_keep, (size_t)m * 4)) ||
      (rc = ensure(op, op->b_opos, (size_t)m * 4)) || (rc = ensure(op, op->b_kpos, (size_t)m * 4)))
    return rc;
  uint32_t *flo = (uint32_t*)op->b_flo.p, *fhi = (uint32_t*)op->b_fhi.p, *fire = (uint32_t*)op->b_fire.p,
           *keep = (uint32_t*)op->b_keep.p, *opos = (uint32_t*)op->b_opos.p, *kpos = (uint32_t*)op->b_kpos.p;
  if (op->fsum_cols && (rc = ensure(op, op->b_fseg, (size_t)m * 4))) return rc;
  hipLaunchKernelGGL(k_ov_frames, dim3(grid_of(m)), dim3(256), 0, op->stream, c, op->map, g, m, flo, fhi, fire, keep,
                     op->fsum_cols ? (uint32_t*)op->b_fseg.p : nullptr);
  if ((rc = excl_scan(op, fire, opos, m)) || (rc = excl_scan(op, keep, kpos, m))) return rc;
  hipLaunchKernelGGL(k_ov_total, dim3(1), dim3(1), 0, op->stream, fire, opos, m, op->tot);
  hipLaunchKernelGGL(k_ov_total, dim3(1), dim3(1), 0, op->stream, keep, kpos, m, op->tot + 1);
  // scans and range-minimum tables, one pass per column / instance
  const int64_t ntiles = (m + OV_TILE - 1) / OV_TILE;
  OScan sc{};
  if ((rc = ensure(op, op->b_thead, (size_t)ntiles * 4))) return rc;
  sc.thead = (const uint32_t*)op->b_thead.p;
  for (int j = 0; j < c.nc; j++) {
    if (!((op->used_cols >> j) & 1)) continue;
    if ((rc = ensure(op, op->b_pnn[j], (size_t)m * 8)) || (rc = ensure(op, op->b_plo[j], (size_t)m * 8)) ||
        (rc = ensure(op, op->b_phi[j], (size_t)m * 8)) || (rc = ensure(op, op->b_tagg[j], (size_t)ntiles * sizeof(SAcc))) ||
        (rc = ensure(op, op->b_carry[j], (size_t)ntiles * sizeof(SAcc))))
      return rc;
    if (ov_float(c.ctype[j])) launch_scan<true>(op, g, j, m, ntiles); else launch_scan<false>(op, g, j, m, ntiles);
    sc.pnn[j] = (const unsigned long long*)op->b_pnn[j].p;
    sc.plo[j] = (const unsigned long long*)op->b_plo[j].p;
    sc.phi[j] = (const long long*)op->b_phi[j].p;
    sc.carry[j] = (const SAcc*)op->b_carry[j].p;
  }
  const int64_t nb = (m + OV_BLOCK - 1) / OV_BLOCK;
  int blevels = 1;
  while ((int64_t(1) << blevels) < nb) blevels++;
  // ROWS frames of at most 64 rows never ask the block table
  const bool need_bt = !(c.kind == FW_OVER_BOUNDED_ROWS && c.prec + 1 <= OV_BLOCK);
  for (int j = 0; j < c.nc; j++) {
    for (int is_max = 0; is_max < 2; is_max++) {
      if (!(((is_max ? op->max_cols : op->min_cols) >> j) & 1)) continue;
      const int q = j * 2 + is_max;
      if ((rc = ensure(op, op->b_rbase[q], (size_t)m * 8)) || (rc = ensure(op, op->b_rst[q], (size_t)m * 8 * OV_LEVELS)) ||
          (rc = ensure(op, op->b_rbt[q], (size_t)nb * 8 * (blevels + 1))))
        return rc;
      int64_t *base = (int64_t*)op->b_rbase[q].p, *stb = (int64_t*)op->b_rst[q].p, *bt = (int64_t*)op->b_rbt[q].p;
      hipLaunchKernelGGL(k_ov_rmq_base, dim3(grid_of(m)), dim3(256), 0, op->stream, g, j, is_max, ov_float(c.ctype[j]) ? 1 : 0,
                         m, base);
      hipLaunchKernelGGL(k_ov_rmq_build, dim3(grid_of(m, OV_RT)), dim3(256), 0, op->stream, (const int64_t*)base, m, m, stb,
                         bt);
      if (need_bt)
        for (int l = 1; l <= blevels; l++)
          hipLaunchKernelGGL(k_ov_rmq_blocks, dim3(grid_of(nb)), dim3(256), 0, op->stream,
                             (const int64_t*)(bt + (int64_t)(l - 1) * nb), bt + (int64_t)l * nb, nb, int64_t(1) << (l - 1));
      ORmq r{base, stb, bt, m, nb};
      (is_max ? sc.mx[j] : sc.mn[j]) = r;
    }
  }
  for (int j = 0; j < c.nc; j++) {  // where a bounded key's Double sum stops being finite (after every scan)
    if (!((op->fsum_cols >> j) & 1)) continue;
    if ((rc = ensure(op, op->b_bad[j], (size_t)m * 4)) || (rc = ensure(op, op->b_bcnt[j], (size_t)m * 4))) return rc;
    hipLaunchKernelGGL(k_ov_nonfinite, dim3(grid_of(m)), dim3(256), 0, op->stream, c, op->map, sc, g, j, m,
                       (const uint32_t*)flo, (const uint32_t*)fhi, (const uint32_t*)fire, (uint32_t*)op->b_bad[j].p);
    if ((rc = excl_scan(op, (const uint32_t*)op->b_bad[j].p, (uint32_t*)op->b_bcnt[j].p, m))) return rc;
  }
  for (int j = 0; j < c.nc; j++) {
    if (!((op->fsum_cols >> j) & 1)) continue;
    sc.bad[j] = (const uint32_t*)op->b_bad[j].p;
    sc.bcnt[j] = (const uint32_t*)op->b_bcnt[j].p;
    sc.fseg = (const uint32_t*)op->b_fseg.p;
  }
  TB_HIP(op, hipMemcpyAsync(htot, op->tot, 16, hipMemcpyDeviceToHost, op->stream));
  TB_HIP(op, hipStreamSynchronize(op->stream));
  const int64_t nfire = (int64_t)htot[0], nkeep = (int64_t)htot[1];
  if ((rc = grow_out(op, op->n_out + nfire))) return rc;  // the row buffer, from the exact count
  hipLaunchKernelGGL(k_ov_eval, dim3(grid_of(m)), dim3(256), 0, op->stream, c, op->map, sc, g, m, flo, fhi, fire, opos,
                     op->n_out, op->ocap, op->out.key, op->out.ts, op->out.ord, op->out.val, op->out.nul);
  hipLaunchKernelGGL(k_ov_state, dim3(grid_of(m)), dim3(256), 0, op->stream, c, op->map, sc, g, m, flo, fhi, fire, op->used_cols);
  hipLaunchKernelGGL(k_ov_retain, dim3(grid_of(m)), dim3(256), 0, op->stream, c, g, other, m, rest, keep, kpos);
  if ((rc = read_ctr(op))) return rc;
  TB_HIP(op, hipGetLastError());
  op->cur ^= 1;
  op->n_store = rest + nkeep;
  op->pending -= nfire;
  op->next_due = op->hctr->due_rest;
  op->hctr->next_due = op->next_due;
  TB_HIP(op, hipMemcpyAsync(&op->ctr->next_due, &op->hctr->next_due, 8, hipMemcpyHostToDevice, op->stream));
  TB_HIP(op, hipStreamSynchronize(op->stream));
  op->n_out += nfire;
  op->fired_total += nfire;
  append_segment(op, call, nfire);
  if (n_rows) *n_rows = nfire;
  return FW_OK;
}

}  // namespace

extern "C" {

int fw_over_create(const fw_over_config* cfg, fw_over** out) {
  if (!cfg || !out) return FW_ERR_ARG;
  *out = nullptr;
  fw_over* op = new fw_over();
  op->cfg = *cfg;
  op->device = cfg->device;
  const fw_over_config& c = *cfg;
  auto fail = [&](int code, const char* msg) {  // as fw_create: the handle carries the message; destroy it
    op->err = msg;
    *out = op;
    return code;
  };
  if (c.kind < FW_OVER_BOUNDED_ROWS || c.kind > FW_OVER_UNBOUNDED_RANGE)
    return fail(FW_ERR_ARG, "kind must be FW_OVER_BOUNDED_ROWS, _BOUNDED_RANGE, _UNBOUNDED_ROWS or _UNBOUNDED_RANGE");
  if (c.kind == FW_OVER_BOUNDED_ROWS && (c.preceding < 0 || c.preceding >= (int64_t(1) << 31)))
    return fail(FW_ERR_ARG, "ROWS BETWEEN n PRECEDING: n must be in [0, 2^31)");
  if (c.kind == FW_OVER_BOUNDED_RANGE && c.preceding < 0)
    return fail(FW_ERR_ARG, "RANGE BETWEEN t PRECEDING: t must be >= 0 ms");
  if (c.key_kind != FW_KEY_LONG && c.key_kind != FW_KEY_INT && c.key_kind != FW_KEY_HASHED)
    return fail(FW_ERR_ARG, "key_kind must be FW_KEY_LONG, FW_KEY_INT or FW_KEY_HASHED");
  if (c.max_parallelism < 1 || c.max_parallelism > 32768 || c.key_group_start < 0 ||
      c.key_group_end < c.key_group_start || c.key_group_end >= c.max_parallelism)
    return fail(FW_ERR_ARG, "max_parallelism must be in [1, 32768] and the KeyGroupRange inside [0, max_parallelism)");
  if (c.row_columns < 1 || c.row_columns > 8) return fail(FW_ERR_ARG, "row_columns must be 1 .. 8");
  if (c.row_aggregates < 1 || c.row_aggregates > 16) return fail(FW_ERR_ARG, "row_aggregates must be 1 .. 16");
  if (c.expected_keys < 0 || c.max_batch < 0) return fail(FW_ERR_ARG, "expected_keys and max_batch must be >= 0");
  for (int j = 0; j < c.row_columns; j++)
    if (c.row_column_type[j] < FW_VAL_I64 || c.row_column_type[j] > FW_VAL_F32)
      return fail(FW_ERR_ARG, "row_column_type must be a FW_VAL_* type");
  for (int q = 0; q < c.row_aggregates; q++) {
    const int fn = c.row_aggregate[q] >> 8, j = c.row_aggregate[q] & 0xff;
    if (fn < FW_ROW_COUNT_STAR || fn > FW_ROW_AVG) return fail(FW_ERR_ARG, "row_aggregate: unknown FW_ROW_* function");
    if (fn == FW_ROW_COUNT_STAR) continue;
    if (j >= c.row_columns) return fail(FW_ERR_ARG, "row_aggregate: column out of range");
    if (c.row_column_type[j] == FW_VAL_F32 && (fn == FW_ROW_SUM || fn == FW_ROW_AVG))
      return fail(FW_ERR_UNSUPPORTED,
                  "SUM / AVG of a Float column over an OVER window is not offered: the reference rounds to float after "
                  "every accumulate and retract, which a parallel frame evaluation cannot reproduce");
  }
  OCfg& d = op->c;
  d.kind = c.kind;
  d.key_kind = c.key_kind;
  d.max_par = c.max_parallelism;
  d.kg0 = c.key_group_start;
  d.nkg = c.key_group_end - c.key_group_start + 1;
  d.nc = c.row_columns;
  d.ns = c.row_aggregates;
  d.prec = c.kind <= FW_OVER_BOUNDED_RANGE ? c.preceding : 0;
  for (int j = 0; j < 8; j++) d.ctype[j] = j < d.nc ? c.row_column_type[j] : 0;
  for (int q = 0; q < 16; q++) d.agg[q] = q < d.ns ? c.row_aggregate[q] : 0;
  for (int q = 0; q < d.ns; q++) {
    const int fn = d.agg[q] >> 8, j = d.agg[q] & 0xff;
    if (fn == FW_ROW_COUNT_STAR) continue;
    op->used_cols |= 1u << j;
    if (fn == FW_ROW_MIN) op->min_cols |= 1u << j;
    if (fn == FW_ROW_MAX) op->max_cols |= 1u << j;
    if ((fn == FW_ROW_SUM || fn == FW_ROW_AVG) && ov_bounded(d) && d.ctype[j] == FW_VAL_F64) op->fsum_cols |= 1u << j;
  }
  *out = op;
  // ---- the GPU from here on
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || c.device < 0 || c.device >= ndev) {
    (void)hipGetLastError();
    return set_err(op, FW_ERR_HIP, "device %d is not available (%d devices)", c.device, ndev);
  }
  TB_HIP(op, hipSetDevice(c.device));
  TB_HIP(op, hipStreamCreateWithFlags(&op->stream, hipStreamNonBlocking));
  TB_HIP(op, hipMalloc(&op->ctr, sizeof(OCtr)));
  TB_HIP(op, hipMalloc(&op->tot, 16));
  TB_HIP(op, hipHostMalloc(&op->hctr, sizeof(OCtr)));
  memset(op->hctr, 0, sizeof(OCtr));
  op->hctr->next_due = LMAX;
  op->hctr->due_rest = LMAX;
  int rc;
  if ((rc = write_ctr(op))) return rc;
  const int64_t mb = c.max_batch > 0 ? c.max_batch : (int64_t(1) << 16);
  if ((rc = grow_map(op, std::max<int64_t>(c.expected_keys, 1024)))) return rc;
  if ((rc = grow_store(op, mb))) return rc;
  op->ready = true;
  return FW_OK;
}

void fw_over_destroy(fw_over* op) {
  if (!op) return;
  if (op->stream) {
    (void)hipSetDevice(op->device);
    (void)hipStreamSynchronize(op->stream);
    free_map(op->map, slot_cols(op));
    for (ORowsD& r : op->store) cols_free(row_cols(op)(r));
    cols_free(out_cols(op)(op->out));
    (void)hipFree(op->ctr);
    (void)hipFree(op->tot);
    (void)hipHostFree(op->hctr);
    (void)hipStreamDestroy(op->stream);
  }
  delete op;
}

const char* fw_over_last_error(const fw_over* op) { return op ? op->err.c_str() : "null handle"; }

int fw_over_push_batch_device(fw_over* op, const int64_t* key, const int64_t* rowtime, const int64_t* cols,
                              const uint8_t* nulls, const int32_t* key_hash, int64_t n) {
  int rc;
  if ((rc = enter_push(op, !key || !rowtime || !cols, key_hash, n)) || (rc = on_device(op))) return rc;
  return do_push(op, key, rowtime, cols, nulls, key_hash, n);
}

int fw_over_push_batch(fw_over* op, const int64_t* key, const int64_t* rowtime, const int64_t* cols,
                       const uint8_t* nulls, const int32_t* key_hash, int64_t n) {
  int rc;
  if ((rc = enter_push(op, !key || !rowtime || !cols, key_hash, n))) return rc;
  if (n == 0) return FW_OK;
  for (int64_t i = 0; i < n; i++)
    if (rowtime[i] == LMIN)
      return set_err(op, FW_ERR_NO_TIMESTAMP, "row %lld has a Long.MIN_VALUE row time; the push was refused", (long long)i);
  if ((rc = on_device(op))) return rc;
  const size_t sz[5] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 8 * op->c.nc, (size_t)n, (size_t)n * 4};
  const void* src[5] = {key, rowtime, cols, nulls, key_hash};
  for (int q = 0; q < 5; q++) {
    if (!src[q]) continue;
    if ((rc = ensure(op, op->b_stage[q], sz[q]))) return rc;
    TB_HIP(op, hipMemcpyAsync(op->b_stage[q].p, src[q], sz[q], hipMemcpyHostToDevice, op->stream));
  }
  TB_HIP(op, hipStreamSynchronize(op->stream));
  return do_push(op, (const int64_t*)op->b_stage[0].p, (const int64_t*)op->b_stage[1].p, (const int64_t*)op->b_stage[2].p,
                 nulls ? (const uint8_t*)op->b_stage[3].p : nullptr, key_hash ? (const int32_t*)op->b_stage[4].p : nullptr, n);
}

int fw_over_advance_watermark(fw_over* op, int64_t wm, int64_t* n_rows) {
  int rc;
  if ((rc = enter(op))) return rc;
  if (wm < op->wm) return set_err(op, FW_ERR_ARG, "watermark %lld is lower than the current %lld", (long long)wm, (long long)op->wm);
  if ((rc = on_device(op))) return rc;
  return do_watermark(op, wm, n_rows);
}

int fw_over_drain(fw_over* op, const fw_over_rows* dst, int64_t* epoch, int64_t cap, int64_t* n) {
  int rc;
  if ((rc = enter(op, !dst || !n || cap < 0)) || (rc = on_device(op))) return rc;
  const OOut& o = op->out;
  return drain_pending(op, {{dst->key, o.key, 8}, {dst->rowtime, o.ts, 8}, {dst->ordinal, o.ord, 8},
                            {dst->values, o.val, (size_t)8 * op->c.ns}, {dst->null_mask, o.nul, 4}},
                       epoch, cap, n);
}

int fw_over_rows_device(fw_over* op, fw_over_rows* rows, int64_t* n) {
  const int rc = enter(op, !rows || !n);
  if (rc) return rc;
  rows->key = op->out.key;
  rows->rowtime = op->out.ts;
  rows->ordinal = op->out.ord;
  rows->values = op->out.val;
  rows->null_mask = op->out.nul;
  *n = op->n_out;
  return FW_OK;
}

int fw_over_clear_pending(fw_over* op) {
  if (!op) return FW_ERR_ARG;
  clear_pending(op);
  return FW_OK;
}

int fw_over_get_stats(fw_over* op, fw_over_stats* out) {
  if (!op || !out) return op ? set_err(op, FW_ERR_ARG, "null argument") : FW_ERR_ARG;
  out->rows_kept = op->kept_total;
  out->late_rows_dropped = op->late_total;
  out->keys = op->nslots;
  out->retained_rows = op->n_store - op->pending;
  out->pending_rows = op->pending;
  out->current_watermark = op->wm;
  out->fired_rows_total = op->fired_total;
  out->pending_output_rows = op->n_out;
  return FW_OK;
}

int fw_over_snapshot_key_group(fw_over* op, int32_t kg, const fw_over_state* dst, int64_t cap_keys, int64_t cap_rows,
                               int64_t* n_keys, int64_t* n_rows) {
  int rc;
  if ((rc = enter_key_group(op, !n_keys || !n_rows, "null argument", kg)) || (rc = on_device(op))) return rc;
  // the key group's slots and rows are picked and compacted on the device: only they cross to the host
  const int64_t ns = op->nslots, n = op->n_store;
  const int w = ov_accw(op->c), nc = op->c.nc;
  *n_keys = *n_rows = 0;
  if (ns == 0) return FW_OK;
  const ORowsD& st = op->store[op->cur];
  Buf fs, ps, fr, pr;  // (freed on every way out)
  if ((rc = ensure(op, fs, (size_t)ns * 4)) || (rc = ensure(op, ps, (size_t)ns * 4)) ||
      (rc = ensure(op, fr, (size_t)std::max<int64_t>(n, 1) * 4)) || (rc = ensure(op, pr, (size_t)std::max<int64_t>(n, 1) * 4)))
    return rc;
  hipLaunchKernelGGL(k_ov_snap_flags, dim3(grid_of(std::max(ns, n))), dim3(256), 0, op->stream, op->map, st, ns, n, kg,
                     (uint32_t*)fs.p, (uint32_t*)fr.p);
  if ((rc = excl_scan(op, (const uint32_t*)fs.p, (uint32_t*)ps.p, ns))) return rc;
  hipLaunchKernelGGL(k_ov_total, dim3(1), dim3(1), 0, op->stream, (const uint32_t*)fs.p, (const uint32_t*)ps.p, ns, op->tot);
  if (n && (rc = excl_scan(op, (const uint32_t*)fr.p, (uint32_t*)pr.p, n))) return rc;
  hipLaunchKernelGGL(k_ov_total, dim3(1), dim3(1), 0, op->stream, (const uint32_t*)fr.p, (const uint32_t*)pr.p, n, op->tot + 1);
  unsigned long long htot[2] = {0, 0};
  if (hipMemcpyAsync(htot, op->tot, 16, hipMemcpyDeviceToHost, op->stream) != hipSuccess ||
      hipStreamSynchronize(op->stream) != hipSuccess)
    return set_err(op, FW_ERR_HIP, "snapshot: reading the counts failed");
  const int64_t nk = (int64_t)htot[0], nr = (int64_t)htot[1];
  *n_keys = nk;
  *n_rows = nr;
  if (!dst || cap_keys < nk || cap_rows < nr || nk == 0) return FW_OK;
  // compacted: per slot {slot, key, last, acc words}, per row {slot, ts, ordinal, columns row-major, nulls}
  Buf d_ss, d_sw, d_rs, d_rw, d_rn;
  const int sw = 2 + w, rw = 2 + nc;
  if ((rc = ensure(op, d_ss, (size_t)nk * 4)) || (rc = ensure(op, d_sw, (size_t)nk * 8 * sw)) ||
      (rc = ensure(op, d_rs, (size_t)std::max<int64_t>(nr, 1) * 4)) ||
      (rc = ensure(op, d_rw, (size_t)std::max<int64_t>(nr, 1) * 8 * rw)) ||
      (rc = ensure(op, d_rn, (size_t)std::max<int64_t>(nr, 1))))
    return rc;
  hipLaunchKernelGGL(k_ov_snap_pack, dim3(grid_of(std::max(ns, n))), dim3(256), 0, op->stream, op->c, op->map, st, ns, n,
                     (const uint32_t*)fs.p, (const uint32_t*)ps.p, (const uint32_t*)fr.p, (const uint32_t*)pr.p,
                     (uint32_t*)d_ss.p, (int64_t*)d_sw.p, (uint32_t*)d_rs.p, (int64_t*)d_rw.p, (uint8_t*)d_rn.p);
  std::vector<uint32_t> hss(nk), hrs(nr);
  std::vector<int64_t> hsw((size_t)nk * sw), hrw((size_t)nr * rw);
  std::vector<uint8_t> hrn(nr);
  bool ok = hipStreamSynchronize(op->stream) == hipSuccess &&
            hipMemcpy(hss.data(), d_ss.p, nk * 4, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(hsw.data(), d_sw.p, (size_t)nk * 8 * sw, hipMemcpyDeviceToHost) == hipSuccess;
  if (ok && nr)
    ok = hipMemcpy(hrs.data(), d_rs.p, nr * 4, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(hrw.data(), d_rw.p, (size_t)nr * 8 * rw, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(hrn.data(), d_rn.p, nr, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) return set_err(op, FW_ERR_HIP, "snapshot: copying the key group's state failed");
  // keys in slot order; a key's rows follow each other in store (arrival) order
  std::unordered_map<uint32_t, int64_t> idx_of;
  idx_of.reserve((size_t)nk * 2);
  std::vector<int64_t> cnt(nk, 0), off(nk + 1, 0);
  for (int64_t i = 0; i < nk; i++) idx_of[hss[i]] = i;
  for (int64_t r = 0; r < nr; r++) cnt[idx_of[hrs[r]]]++;
  for (int64_t i = 0; i < nk; i++) {
    off[i + 1] = off[i] + cnt[i];
    dst->key[i] = hsw[(size_t)i * sw];
    dst->last_ts[i] = ov_bounded(op->c) ? hsw[(size_t)i * sw + 1] : 0;
    for (int q = 0; q < w; q++) dst->acc[i * w + q] = hsw[(size_t)i * sw + 2 + q];
    dst->n_rows[i] = cnt[i];
  }
  std::vector<int64_t> fill(off.begin(), off.end() - 1);
  for (int64_t r = 0; r < nr; r++) {
    const int64_t d = fill[idx_of[hrs[r]]]++;
    dst->ts[d] = hrw[(size_t)r * rw];
    dst->ordinal[d] = hrw[(size_t)r * rw + 1];
    dst->nulls[d] = hrn[r];
    for (int j = 0; j < nc; j++) dst->cols[d * nc + j] = hrw[(size_t)r * rw + 2 + j];
  }
  return FW_OK;
}

int fw_over_restore_key_group(fw_over* op, int32_t kg, const fw_over_state* src, int64_t n_keys, int64_t n_rows) {
  int rc;
  if ((rc = enter_key_group(op, n_keys < 0 || n_rows < 0, "bad argument", kg))) return rc;
  if (n_keys == 0) return n_rows == 0 ? FW_OK : set_err(op, FW_ERR_ARG, "rows without keys");
  if (!src || !src->key || !src->last_ts || !src->acc || !src->n_rows ||
      (n_rows > 0 && (!src->ts || !src->ordinal || !src->cols || !src->nulls)))
    return set_err(op, FW_ERR_ARG, "null column");
  if ((rc = on_device(op))) return rc;
  const OCfg& c = op->c;
  const int w = ov_accw(c), nc = c.nc;
  std::unordered_set<int64_t> seen;
  if ((rc = check_restored_keys(op, c, kg, src->key, src->n_rows, n_keys, n_rows, [](int64_t) { return FW_OK; })) ||
      (rc = check_restored_unique(op, src->key, n_keys, seen)))
    return rc;
  {
    std::vector<int64_t> skey(op->nslots);
    if (op->nslots) TB_HIP(op, hipMemcpy(skey.data(), op->map.skey, op->nslots * 8, hipMemcpyDeviceToHost));
    for (int64_t k : skey)
      if (seen.count(k)) return set_err(op, FW_ERR_STATE, "key %lld already has state in the handle", (long long)k);
  }
  if ((rc = grow_store(op, op->n_store + n_rows))) return rc;
  if ((rc = grow_map(op, op->nslots + n_keys))) return rc;
  // rows in ordinal order (the store keeps a key's rows in arrival order), each with its key
  std::vector<int64_t> rkey(n_rows), order(n_rows);
  int64_t pend = 0, due = LMAX, max_ord = -1;
  {
    int64_t r = 0;
    for (int64_t i = 0; i < n_keys; i++)
      for (int64_t q = 0; q < src->n_rows[i]; q++, r++) {
        rkey[r] = src->key[i];
        order[r] = r;
        if (src->ts[r] == LMIN) return set_err(op, FW_ERR_NO_TIMESTAMP, "a restored row has a Long.MIN_VALUE row time");
        if (!ov_bounded(c) || src->ts[r] > src->last_ts[i]) {
          pend++;
          due = std::min(due, src->ts[r]);
        }
        max_ord = std::max(max_ord, src->ordinal[r]);
      }
  }
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return src->ordinal[a] < src->ordinal[b]; });
  std::vector<int64_t> hk(n_rows), ht(n_rows), ho(n_rows), hc((size_t)n_rows * nc);
  std::vector<uint8_t> hn(n_rows);
  for (int64_t d = 0; d < n_rows; d++) {
    const int64_t r = order[d];
    hk[d] = rkey[r];
    ht[d] = src->ts[r];
    ho[d] = src->ordinal[r];
    hn[d] = src->nulls[r];
    for (int j = 0; j < nc; j++) hc[(size_t)d * nc + j] = src->cols[r * nc + j];
  }
  Buf bk, bl, ba, rk, rt, ro, rcv, rn;
  auto up = [&](Buf& b, const void* p, size_t bytes) -> int {
    if (bytes == 0) return FW_OK;
    int e = ensure(op, b, bytes);
    if (e) return e;
    if (hipMemcpy(b.p, p, bytes, hipMemcpyHostToDevice) != hipSuccess) return set_err(op, FW_ERR_HIP, "hipMemcpy failed");
    return FW_OK;
  };
  rc = up(bk, src->key, n_keys * 8);
  if (!rc) rc = up(bl, src->last_ts, n_keys * 8);
  if (!rc) rc = up(ba, src->acc, (size_t)n_keys * 8 * w);
  if (!rc) rc = up(rk, hk.data(), n_rows * 8);
  if (!rc) rc = up(rt, ht.data(), n_rows * 8);
  if (!rc) rc = up(ro, ho.data(), n_rows * 8);
  if (!rc) rc = up(rcv, hc.data(), (size_t)n_rows * 8 * nc);
  if (!rc) rc = up(rn, hn.data(), n_rows);
  if (!rc) {
    hipLaunchKernelGGL(k_ov_restore_keys, dim3(grid_of(n_keys)), dim3(256), 0, op->stream, c, op->map, op->ctr, kg,
                       (const int64_t*)bk.p, (const int64_t*)bl.p, (const int64_t*)ba.p, n_keys);
    if (n_rows)
      hipLaunchKernelGGL(k_ov_restore_rows, dim3(grid_of(n_rows)), dim3(256), 0, op->stream, c, op->map, op->store[op->cur],
                         op->n_store, (const int64_t*)rk.p, (const int64_t*)rt.p, (const int64_t*)ro.p,
                         (const int64_t*)rcv.p, (const uint8_t*)rn.p, n_rows);
    rc = read_ctr(op);
  }
  if (rc) return rc;
  op->nslots = op->hctr->nslots;
  op->n_store += n_rows;
  op->pending += pend;
  op->next_due = std::min(op->next_due, due);
  op->hctr->next_due = op->next_due;
  if ((rc = write_ctr(op))) return rc;
  op->ord_base = std::max(op->ord_base, max_ord + 1);
  return FW_OK;
}

}  // extern "C"
