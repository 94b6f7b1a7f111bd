// sanitize_main.cpp — ASan + UBSan driver (TEST INFRASTRUCTURE ONLY; SURVEY §5 "Race detection /
// sanitizers": test the C++ under ASan/UBSan, Java's signed-overflow semantics emulated explicitly).
// Built by `make -C oracle sanitize` with -fsanitize=address,undefined and run by tests/test_sanitizers.py.
// It drives the oracle through every operator shape (tumbling / sliding / sessions, lateness, purging,
// side output, first-element, minBy/maxBy, HyperLogLog, t-digest, count windows, the multi-threaded
// baseline) on a seeded stream with extreme keys and timestamps, and checks the host-side arithmetic the
// library shares with the device code (make_div_inv, flink_amd/csrc/fw_internal.h) against 128-bit division, and
// at both ends of the long range the window start, the host's FW_ERR_TIME_RANGE refusals and the compact records' base
// (flink_amd/csrc/fw_range.h) against 128-bit restatements and the oracle.  It also drives the wire oracle
// (wire_oracle.cpp): a mixed stream cut at every byte (each prefix in a heap block of exactly its size, so a read
// past it is seen), corrupt String records, and rows whose `end` and NaN sums sit at the ends of their ranges.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../flink_amd/csrc/fw_internal.h"
#include "../flink_amd/csrc/fw_range.h"
#include "window_oracle.h"
#include "wire_oracle.h"

static uint64_t sm(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the quotient the device computes from (m, l): t1 = mulhi(m, n); (t1 + ((n - t1) >> 1)) >> (l - 1); l == 0: d == 1
static uint64_t div_inv_host(uint64_t n, uint64_t m, int32_t l) {
  if (l == 0) return n;
  const uint64_t t1 = (uint64_t)(((unsigned __int128)m * n) >> 64);
  return (t1 + ((n - t1) >> 1)) >> (l - 1);
}

static int check_div_inv() {
  int bad = 0;
  std::vector<uint64_t> ds = {1, 2, 3, 7, 1000, 60000, 1000003, 86400000ull, (1ull << 40) + 5, ~0ull >> 1,
                              (1ull << 32) + 1, (1ull << 40) + 15, (1ull << 61) + 1, (1ull << 62) + 1};
  for (int k = 2; k <= 62; k++) {  // 2^k - 1 and 2^k + 1
    ds.push_back((1ull << k) - 1);
    ds.push_back((1ull << k) + 1);
  }
  const uint64_t top = 1ull << 63;
  for (uint64_t d : ds) {
    uint64_t m;
    int32_t l;
    make_div_inv(d, &m, &l);
    if ((d == 1) != (l == 0)) bad++;
    if (d == (1ull << 61) + 1 && l != 62) bad++;
    if (d == (1ull << 62) + 1 && l != 63) bad++;
    std::vector<uint64_t> ns = {top, top - 1, top + 1};
    // the multiples of d next to 2^63 (|Long.MIN_VALUE|, the largest dividend jrem forms) and to 2^64, and their neighbours
    for (uint64_t q : {(uint64_t)(top / d), (uint64_t)(top / d + 1), (uint64_t)(~0ull / d)})
      for (int e = -1; e <= 1; e++)
        if (q >= 1 && q <= ~0ull / d) ns.push_back(q * d + (uint64_t)(int64_t)e);
    for (int i = 0; i < 20000; i++)
      ns.push_back(i < 10 ? (uint64_t)i : (i < 20 ? ~0ull - (uint64_t)(i - 10) : sm((uint64_t)i * 7919u + d)));
    for (uint64_t n : ns)
      if (div_inv_host(n, m, l) != n / d) bad++;
  }
  return bad;
}

// the composition the device code makes of it (flink_amd/csrc/fw_device.hip jrem / wstart): |t| with the dividend's
// sign, also for Long.MIN_VALUE, against 128-bit truncating arithmetic wrapped to 64 bits
static int check_window_start() {
  int bad = 0;
  const int64_t sizes[] = {1, 3, 7, 1000, 1023, 1025, 1000003, (1ll << 32) + 1, (1ll << 40) + 15, (1ll << 61) + 1,
                           (1ll << 62) + 1};
  for (int64_t d : sizes) {
    uint64_t m;
    int32_t l;
    make_div_inv((uint64_t)d, &m, &l);
    const int64_t offs[] = {0, d - 1, -(d - 1), -28800000};
    for (int64_t off : offs) {
      for (int i = 0; i < 4000; i++) {
        int64_t ts;
        if (i < 21) ts = (int64_t)((uint64_t)off + (uint64_t)((i / 3 - 3) * (__int128)d) + (uint64_t)(int64_t)(i % 3 - 1));
        else if (i < 24) ts = INT64_MIN + (i - 21);
        else if (i < 27) ts = INT64_MAX - (i - 24);
        else ts = (int64_t)sm((uint64_t)i * 104729u + (uint64_t)d) >> (i % 40);
        const int64_t t = (int64_t)((uint64_t)ts - (uint64_t)off + (uint64_t)d);
        const uint64_t u = t < 0 ? (uint64_t)0 - (uint64_t)t : (uint64_t)t;
        const uint64_t r = u - div_inv_host(u, m, l) * (uint64_t)d;
        const int64_t rem = t < 0 ? -(int64_t)r : (int64_t)r;
        const int64_t got = (int64_t)((uint64_t)ts - (uint64_t)rem);
        const __int128 want_rem = (__int128)t % (__int128)d;  // (C++ truncates as Java does)
        if (rem != (int64_t)want_rem || got != oracle_window_start(ts, off, d)) bad++;
      }
    }
  }
  return bad;
}

// ---- the ends of the long range (DESIGN.md "Event-time arithmetic"): every timestamp within `span` of Long.MAX_VALUE
// and of Long.MIN_VALUE
static const int64_t END_SPAN = 6000;
template <class F>
static void for_end_timestamps(F f) {
  for (int64_t d = 0; d <= END_SPAN; d++) {
    f(INT64_MAX - d);
    f(INT64_MIN + d);
  }
}
// the reciprocal remainder and the window start where ts - offset, + size or the start itself wraps
static int check_window_start_at_the_ends() {
  int bad = 0;
  const int64_t cfgs[][2] = {{1000, 0}, {1000, 1}, {1000, 999}, {1000, 808}, {1000, 308}, {2500, 0}, {500, 308},
                             {700, 1}, {7, 3}, {1000003, 17}, {(1ll << 40) + 15, 12345}, {(1ll << 61) + 1, 5}};
  for (auto& c : cfgs) {
    const int64_t d = c[0], off = c[1];
    uint64_t m;
    int32_t l;
    make_div_inv((uint64_t)d, &m, &l);
    for_end_timestamps([&](int64_t ts) {
      const int64_t t = fw_wadd(fw_wsub(ts, off), d);
      const uint64_t u = t < 0 ? (uint64_t)0 - (uint64_t)t : (uint64_t)t;
      const uint64_t r = u - div_inv_host(u, m, l) * (uint64_t)d;
      const int64_t rem = t < 0 ? -(int64_t)r : (int64_t)r;
      if (rem != (int64_t)((__int128)t % (__int128)d) || fw_wsub(ts, rem) != oracle_window_start(ts, off, d)) bad++;
    });
  }
  return bad;
}
// SlidingEventTimeWindows.assignWindows on 128-bit ints that are wrapped to a long after every step, for at most
// `cap` + 1 windows: the count, whether the newest end wrapped, whether the walk ran past the cap
struct RefWalk {
  int k;
  bool newest_wraps, runaway;
};
static int64_t wrap128(__int128 x) { return (int64_t)(uint64_t)(unsigned __int128)x; }
static RefWalk ref_walk(int64_t ts, int64_t size, int64_t slide, int64_t off, int cap) {
  const int64_t t = wrap128((__int128)wrap128((__int128)ts - off) + slide);
  const int64_t last = wrap128((__int128)ts - (int64_t)((__int128)t % slide)), lo = wrap128((__int128)ts - size);
  RefWalk w{0, (__int128)last + size > (__int128)INT64_MAX, false};
  for (int64_t s = last; s > lo; s = wrap128((__int128)s - slide)) {
    if (w.k == cap) {
      w.runaway = true;
      break;
    }
    w.k++;
  }
  return w;
}
// the host's refusals (fw_range.h: fw_time_range_record, fw_range_guards, fw_sliding_runaway) against that walk and
// against the oracle, which returns OR_ERR_RUNAWAY on exactly the runaway set
static int check_time_range() {
  int bad = 0;
  const int64_t cfgs[][3] = {{2500, 1000, 0}, {2500, 1000, 808}, {2500, 1000, 308}, {3000, 1000, 0}, {3000, 500, 1},
                             {700, 1000, 0}, {1000, 1000, 999}, {7, 3, 2}};
  for (auto& c : cfgs) {
    const int64_t size = c[0], slide = c[1], off = c[2];
    const int cap = (int)(size / slide + (size % slide != 0) + 1);
    int64_t glo, ghi;
    fw_range_guards(size, slide, &glo, &ghi);
    oracle_cfg oc{};
    oc.assigner = OR_SLIDING;
    oc.size = size;
    oc.slide = slide;
    oc.offset = off;
    int n_run = 0;
    for_end_timestamps([&](int64_t ts) {
      if (ts == INT64_MIN) return;
      const RefWalk w = ref_walk(ts, size, slide, off, cap);
      const fw_range_cfg win{size, slide, off, cap, false, false}, td{size, slide, off, cap, false, true};
      const fw_range_cfg pane{size, slide, off, cap, true, false};
      if (fw_time_range_record(win, ts) != w.runaway) bad++;
      if (fw_sliding_runaway(size, slide, off, cap, ts) != w.runaway) bad++;
      if (fw_time_range_record(td, ts) != (w.runaway || (w.k > 1 && w.newest_wraps))) bad++;
      const bool t_wraps = (__int128)wrap128((__int128)ts - off) + slide > (__int128)INT64_MAX;
      const bool bottom = (__int128)ts - size - 2 * (__int128)slide < (__int128)INT64_MIN;
      if (fw_time_range_record(pane, ts) != (w.newest_wraps || t_wraps || bottom)) bad++;
      // nothing between the guards is ever refused, so whatever is refused lies at or beyond one of them
      if ((fw_time_range_record(win, ts) || fw_time_range_record(td, ts) || fw_time_range_record(pane, ts)) &&
          ts > glo && ts < ghi)
        bad++;
      if (w.runaway || (uint64_t)ts - (uint64_t)INT64_MIN == (uint64_t)(size - 1) || ts == INT64_MAX) {  // the oracle agrees on the set and its edges
        void* op = oracle_create(&oc);
        const int64_t k = 1, v = 1;
        if ((oracle_process(op, &k, &ts, &v, 1) == OR_ERR_RUNAWAY) != w.runaway) bad++;
        oracle_destroy(op);
      }
      n_run += w.runaway;
    });
    if (size == 2500 && off == 0 && n_run != 808) bad++;  // ts - Long.MIN_VALUE in [2500, 3307]
    for (int i = 0; i < 2000; i++) {  // and timestamps anywhere else are taken
      const int64_t ts = (int64_t)sm((uint64_t)i * 7919u + (uint64_t)size) >> (i % 30);
      if (ts > glo && ts < ghi && (fw_time_range_record(fw_range_cfg{size, slide, off, cap, true, true}, ts) ||
                                   fw_sliding_runaway(size, slide, off, cap, ts)))
        bad++;
    }
  }
  // sizes for which size + 2 slide leaves the long range: the guards saturate, nothing overflows
  for (int64_t size : {(int64_t)((1ll << 62) + 1), (int64_t)INT64_MAX}) {
    int64_t glo, ghi;
    fw_range_guards(size, size, &glo, &ghi);
    if (glo < -1 || ghi > 0) bad++;
    for (int64_t ts : {(int64_t)(INT64_MIN + 1), (int64_t)-1, (int64_t)0, (int64_t)INT64_MAX}) {
      (void)fw_time_range_record(fw_range_cfg{size, size, 0, 2, true, false}, ts);
      (void)fw_sliding_runaway(size, size, 0, 2, ts);
    }
  }
  return bad;
}
// the compact records' base with watermarks at both ends: a base is on the grid, 2^(log_s - 1) steps below the
// watermark's grid point, and refused exactly when that point leaves the long range
static int check_compact_base() {
  int bad = 0;
  const int64_t cfgs[][2] = {{1000, 0}, {1000, 808}, {1000, 999}, {100, 1}, {(1ll << 40) + 15, 7}, {(1ll << 62) + 1, 0}};
  for (auto& c : cfgs) {
    const int64_t step = c[0], off = c[1];
    for (int log_s : {1, 3, 8, 12}) {
      auto one = [&](int64_t wm) {
        int64_t base = 0;
        const bool ok = fw_compact_base(wm, off, step, log_s, &base);
        __int128 g = (__int128)wm - off;  // the watermark's grid point, by floor division on 128 bits
        g = g - ((g % step) + step) % step + off;
        const __int128 want = g - ((__int128)1 << (log_s - 1)) * step;
        const bool fits = want >= (__int128)INT64_MIN && want <= (__int128)INT64_MAX;
        if (ok != fits || (ok && (__int128)base != want)) bad++;
      };
      for_end_timestamps(one);
      for (int64_t wm : {(int64_t)0, (int64_t)-1, (int64_t)1, off, (int64_t)(off - 1)}) one(wm);
    }
  }
  return bad;
}

static void run(oracle_cfg cfg, int n, uint64_t seed) {
  void* op = oracle_create(&cfg);
  std::vector<int64_t> k(n), t(n), v(n);
  int64_t mx = INT64_MIN + 5000;
  for (int b = 0; b < 4; b++) {
    for (int i = 0; i < n; i++) {
      const uint64_t r = sm(seed ^ ((uint64_t)(b * n + i) << 2));
      k[i] = (int64_t)(r % 97) - 48;
      if (i % 31 == 0) k[i] = (i & 1) ? INT64_MAX : INT64_MIN;  // extreme keys
      t[i] = 1000000 + (int64_t)((b * n + i) / 4) - (int64_t)(sm(r) % 300);
      if (b == 3 && i % 53 == 0) t[i] = INT64_MAX - 1750 + (int64_t)(r % 100);  // cleanup-time overflow
      const int64_t x = (int64_t)sm(r + 1);
      if (cfg.value_type == OR_VAL_F64) {
        const double d = (double)(x % 1000000) / 7.0;
        memcpy(&v[i], &d, 8);
      } else {
        v[i] = cfg.value_type == OR_VAL_I32 ? (int64_t)(int32_t)x : x;
      }
      if (t[i] > mx) mx = t[i];
    }
    oracle_process(op, k.data(), t.data(), v.data(), n);
    oracle_watermark(op, mx - 200);
  }
  oracle_watermark(op, INT64_MAX);
  std::vector<oracle_row> rows((size_t)oracle_num_rows(op));
  if (!rows.empty()) oracle_get_rows(op, rows.data());
  if (cfg.aggregate == OR_AGG_TDIGEST && !rows.empty()) {
    std::vector<double> s(64);
    std::vector<int64_t> w(64);
    oracle_row_digest(op, 0, s.data(), w.data(), 64);
  }
  std::vector<oracle_side_row> side((size_t)oracle_num_side_rows(op));
  if (!side.empty()) oracle_get_side_rows(op, side.data());
  oracle_destroy(op);
}

// ---- the wire oracle
static void put_bytes(std::vector<uint8_t>& v, std::initializer_list<int> bs) {
  for (int b : bs) v.push_back((uint8_t)b);
}
// one element: the 4-byte length of the parts' bytes, then those bytes
static std::vector<uint8_t> framed(std::initializer_list<std::initializer_list<int>> parts) {
  std::vector<uint8_t> v = {0, 0, 0, 0};
  for (const auto& p : parts) put_bytes(v, p);
  v[3] = (uint8_t)(v.size() - 4);
  return v;
}
// decode `n` bytes from a heap block of exactly n bytes
static int decode_exact(const uint8_t* src, int64_t n, const oracle_wire_layout* L, oracle_wire_stats* st, int64_t* recs) {
  uint8_t* blk = (uint8_t*)malloc(n ? (size_t)n : 1);
  if (n) memcpy(blk, src, (size_t)n);
  const int64_t cap = n / 5 + 1;
  std::vector<int64_t> k((size_t)cap), t((size_t)cap), v((size_t)cap);
  std::vector<int32_t> h((size_t)cap);
  const int rc = oracle_wire_decode_keyed(n ? blk : nullptr, n, L, k.data(), h.data(), t.data(), v.data(), cap, st);
  if (recs) *recs = st->records;
  free(blk);
  return rc;
}
static int check_wire() {
  int bad = 0;
  const oracle_wire_layout F3{3, {OR_WIRE_LONG, OR_WIRE_LONG, OR_WIRE_INT}, {OR_ROLE_KEY, OR_ROLE_SKIP, OR_ROLE_VALUE}};
  const oracle_wire_layout S4{4, {OR_WIRE_LONG, OR_WIRE_STRING, OR_WIRE_STRING, OR_WIRE_INT},
                              {OR_ROLE_SKIP, OR_ROLE_KEY, OR_ROLE_SKIP, OR_ROLE_VALUE}};
  const oracle_wire_layout S2{2, {OR_WIRE_STRING, OR_WIRE_INT}, {OR_ROLE_KEY, OR_ROLE_VALUE}};
  {  // a mixed stream of every element kind, cut at every byte: records and consumed never shrink, nothing is corrupt
    std::vector<uint8_t> b(64 * 40);
    int64_t n = 0;
    for (int i = 0; i < 60; i++) {
      const int64_t f[3] = {i % 2 ? INT64_MIN : INT64_MAX - i, -i, i * 77};
      switch (i % 5) {
        case 0: n += oracle_wire_put_record(&F3, 1, i % 10 ? i : INT64_MIN, f, b.data() + n); break;
        case 1: n += oracle_wire_put_record(&F3, 0, 0, f, b.data() + n); break;
        case 2: n += oracle_wire_put_watermark(i == 57 ? INT64_MIN : i, b.data() + n); break;
        case 3: n += oracle_wire_put_latency(i, INT64_MIN, INT64_MAX, i, b.data() + n); break;
        default: n += oracle_wire_put_status(i == 59 ? INT32_MIN : -(i & 1), b.data() + n); break;
      }
    }
    int64_t last_recs = 0, last_cons = 0;
    for (int64_t cut = 0; cut <= n; cut++) {
      oracle_wire_stats st;
      int64_t recs = 0;
      if (decode_exact(b.data(), cut, &F3, &st, &recs) != 0) bad++;
      if (recs < last_recs || st.consumed < last_cons || st.consumed > cut) bad++;
      last_recs = recs;
      last_cons = st.consumed;
      if (cut == n && (st.consumed != n || recs != 24 || st.watermark != INT64_MIN || st.status != INT32_MIN)) bad++;
    }
    for (int tag : {5, 0x80, 0xff}) {  // an unknown tag, also as the very last byte of the block
      std::vector<uint8_t> c(b.begin(), b.begin() + 33);
      put_bytes(c, {0, 0, 0, 1, tag});
      oracle_wire_stats st;
      if (decode_exact(c.data(), (int64_t)c.size(), &F3, &st, nullptr) != -1 || st.bad_tag != (int8_t)tag || st.consumed != 33) bad++;
    }
    std::vector<uint8_t> e = {0, 0, 0, 0};  // an empty element
    oracle_wire_stats st;
    if (decode_exact(e.data(), 4, &F3, &st, nullptr) != -1 || st.bad_tag != -3) bad++;
  }
  {  // String records: good ones cut at every byte, then the corruptions (each must be refused, none read past its end)
    const std::initializer_list<int> ts9 = {0, 0, 0, 0, 0, 0, 0, 0, 9};  // tag 0 and its timestamp
    std::vector<uint8_t> g = framed({ts9, {1, 2, 3, 4, 5, 6, 7, 8, 3, 'a', 0xe5, 0xcb, 0x01, 0, 0, 0, 0, 7}});
    const std::vector<uint8_t> g2 = framed({{1, 1, 2, 3, 4, 5, 6, 7, 8, 1, 4, 0xff, 0xff, 0x03, 'x', 'y', 0, 0, 0, 7}});
    g.insert(g.end(), g2.begin(), g2.end());
    for (int64_t cut = 0; cut <= (int64_t)g.size(); cut++) {
      oracle_wire_stats st;
      int64_t recs = 0;
      if (decode_exact(g.data(), cut, &S4, &st, &recs) != 0) bad++;
      if (cut == (int64_t)g.size() && (recs != 2 || st.consumed != cut)) bad++;
    }
    const std::vector<std::vector<uint8_t>> corrupt = {
        framed({ts9, {3, 'a', 0xe5}}),                                               // a char's varint runs past the element
        framed({ts9, {0x83}}),                                                       // the length's varint does
        framed({ts9, {3, 'a', 'b', 0, 0, 0, 7, 0}}),                                 // the String ends before the element
        framed({ts9, {6, 'a', 'b'}}),                                                // ... and after it
        framed({ts9, {2, 0x81, 0x80, 0x80, 0x80, 0x80, 0, 0, 0, 0, 7}}),             // a fifth byte that continues
        framed({ts9, {2, 0x81, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0, 0, 0, 0, 7}}),
        framed({ts9, {0xff, 0xff, 0xff, 0xff, 0x0f, 'a', 'b', 0, 0, 0, 7}}),         // a huge length
        framed({{0, 1, 2}}),                                                         // no room for the timestamp
    };
    for (const auto& v : corrupt) {
      oracle_wire_stats st;
      if (decode_exact(v.data(), (int64_t)v.size(), &S2, &st, nullptr) != -1 || st.bad_tag != -2 || st.consumed != 0) bad++;
    }
    const std::vector<uint8_t> nk = framed({ts9, {0, 0, 0, 0, 7}});  // a null String key
    oracle_wire_stats st;
    if (decode_exact(nk.data(), (int64_t)nk.size(), &S2, &st, nullptr) != -1 || st.bad_tag != -4) bad++;
  }
  {  // encode: `end` at both ends of the long range (end - 1 wraps as Java's does), NaN and out-of-range sums
    const oracle_wire_layout out{6, {OR_WIRE_DOUBLE, OR_WIRE_FLOAT, OR_WIRE_LONG, OR_WIRE_INT, OR_WIRE_SHORT, OR_WIRE_BYTE},
                                 {OR_ROLE_SUM, OR_ROLE_SUM, OR_ROLE_SUM, OR_ROLE_MIN, OR_ROLE_MAX, OR_ROLE_END}};
    const uint64_t sums[] = {0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff0000000000001ull, 0xffffffffffffffffull,
                             0x43e0000000000000ull /* 2^63 */, 0xc3e0000000000001ull, 0x7fe1ccf385ebc8a0ull /* 1e308 */,
                             0xfff0000000000000ull, 0x0000000000000001ull, 0x47efffffe0000000ull /* FLT_MAX */};
    const int64_t ends[] = {3000, INT64_MAX, INT64_MIN, 0, INT64_MIN + 1};
    std::vector<oracle_row> rows;
    for (uint64_t sb : sums)
      for (int64_t e : ends) {
        oracle_row r{};
        r.end = e;
        r.start = e;
        memcpy(&r.sum, &sb, 8);
        r.min = r.sum;
        r.max = r.sum;
        rows.push_back(r);
      }
    for (int f64 = 0; f64 <= 1; f64++) {
      const int64_t S = 13 + 27, n = (int64_t)rows.size();
      uint8_t* o = (uint8_t*)malloc((size_t)(n * S));
      if (oracle_wire_encode(&out, rows.data(), n, f64, o, n * S) != n * S) bad++;
      if (oracle_wire_encode(&out, rows.data(), n, f64, o, n * S - 1) != -1) bad++;
      for (int64_t r = 0; r < n; r++) {
        uint64_t ts = 0, d = 0;
        for (int i = 0; i < 8; i++) {
          ts = (ts << 8) | o[r * S + 5 + i];
          d = (d << 8) | o[r * S + 13 + i];
        }
        const int64_t e = rows[(size_t)r].end;
        if (ts != (e == INT64_MAX ? (uint64_t)e : (uint64_t)e - 1u)) bad++;
        const bool nan = (d & 0x7ff0000000000000ull) == 0x7ff0000000000000ull && (d & 0x000fffffffffffffull);
        if (nan && d != 0x7ff8000000000000ull) bad++;  // Double.doubleToLongBits
      }
      free(o);
    }
  }
  return bad;
}

int main() {
  const int bad_wire = check_wire();
  if (bad_wire) {
    fprintf(stderr, "the wire oracle: %d wrong\n", bad_wire);
    return 1;
  }
  const int bad = check_div_inv();
  if (bad) {
    fprintf(stderr, "make_div_inv: %d wrong quotients\n", bad);
    return 1;
  }
  const int bad_ws = check_window_start();
  if (bad_ws) {
    fprintf(stderr, "window start through the reciprocal: %d wrong\n", bad_ws);
    return 1;
  }
  const int bad_ends = check_window_start_at_the_ends();
  const int bad_range = check_time_range();
  const int bad_base = check_compact_base();
  if (bad_ends || bad_range || bad_base) {
    fprintf(stderr, "the ends of the long range: %d wrong window starts, %d wrong refusals, %d wrong compact bases\n",
            bad_ends, bad_range, bad_base);
    return 1;
  }
  oracle_cfg base{};
  base.td_delta = 100;
  base.td_q[0] = 0.5;
  base.td_q[1] = 0.9;
  base.td_q[2] = 0.99;
  auto cfg = [&](int a, int vt, int64_t size, int64_t slide, int64_t gap, int64_t late, int purge, int side, int agg) {
    oracle_cfg c = base;
    c.assigner = a;
    c.value_type = vt;
    c.size = size;
    c.slide = slide;
    c.gap = gap;
    c.lateness = late;
    c.purging = purge;
    c.side_output = side;
    c.aggregate = agg;
    c.hll_p = 10;
    return c;
  };
  run(cfg(OR_TUMBLING, OR_VAL_I64, 1000, 1000, 0, 0, 0, 0, OR_AGG_COUNT_SUM_MIN_MAX), 3000, 1);
  run(cfg(OR_TUMBLING, OR_VAL_I32, 1000, 1000, 0, 700, 1, 1, OR_AGG_FIRST), 3000, 2);
  run(cfg(OR_SLIDING, OR_VAL_F64, 3000, 1000, 0, 0, 0, 0, OR_AGG_COUNT_SUM_MIN_MAX), 2000, 3);
  run(cfg(OR_SLIDING, OR_VAL_I64, 2000, 500, 0, 300, 0, 1, OR_AGG_MINBY), 2000, 4);
  run(cfg(OR_SESSION, OR_VAL_F64, 0, 0, 300, 200, 1, 1, OR_AGG_MAXBY), 3000, 5);
  run(cfg(OR_SESSION, OR_VAL_I64, 0, 0, 50, 0, 0, 0, OR_AGG_FIRST_MAX), 3000, 6);
  run(cfg(OR_TUMBLING, OR_VAL_I64, 1000, 1000, 0, 0, 0, 0, OR_AGG_HLL), 3000, 7);
  run(cfg(OR_TUMBLING, OR_VAL_F64, 1000, 1000, 0, 0, 0, 0, OR_AGG_TDIGEST), 6000, 8);
  {  // count windows (a14)
    void* cw = oracle_count_create(10, 5, 1, OR_VAL_I32);
    std::vector<int64_t> k(5000), v(5000);
    for (int i = 0; i < 5000; i++) {
      k[i] = (int64_t)(sm(i) % 170);
      v[i] = 1;
    }
    oracle_count_process(cw, k.data(), v.data(), 5000);
    std::vector<oracle_row> rows((size_t)oracle_count_num_rows(cw));
    if (!rows.empty()) oracle_count_get_rows(cw, rows.data());
    oracle_count_destroy(cw);
  }
  {  // the multi-threaded CPU baseline (p = 4 subtasks)
    oracle_cfg c = cfg(OR_TUMBLING, OR_VAL_I64, 1000, 1000, 0, 0, 0, 0, OR_AGG_COUNT_SUM_MIN_MAX);
    const int n = 40000;
    std::vector<int64_t> k(n), t(n), v(n), wms(4);
    for (int i = 0; i < n; i++) {
      k[i] = (int64_t)(sm(i) % 1000);
      t[i] = i / 10;
      v[i] = (int64_t)sm(i + 1);
    }
    for (int b = 0; b < 4; b++) wms[b] = (int64_t)((b + 1) * n / 4) / 10 - 200;
    int64_t late = 0;
    oracle_run_parallel(&c, k.data(), t.data(), v.data(), n, n / 4, wms.data(), 4, 128, 4, &late);
  }
  printf("sanitized run ok\n");
  return 0;
}
