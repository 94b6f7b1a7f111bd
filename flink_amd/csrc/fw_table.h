// fw_table.h — what the Table API handles share (fw_over.hip and fw_tjoin.hip include it, nothing else does):
//   device: the key map (lock-free find-or-claim, rebuilt on growth) and the wave helpers
//   host:   the handle base (error text, stream, scratch, pending output), column sets that grow by doubling,
//           rocprim scan / sort wrappers, the drain, and the heads of the entry points and of a restore.
// Everything sits in the translation unit's anonymous namespace: each of the two holds its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/flink_window.h"
#include "fw_keygroup.h"

namespace {

constexpr int64_t LMAX = INT64_MAX;
constexpr int64_t LMIN = INT64_MIN;
#include "fw_jmath.h"

// ---------------------------------------------------------------- key map
// An open-addressing table (load <= 1/2) from a key to its slot, the index of the key's state in the per-slot
// columns.  A handle derives its map from this and adds its own per-slot columns.
struct KeyMap {
  int64_t* mkey;
  uint32_t* mstate;  // 0 empty, 1 being published, 2 taken
  uint32_t* mslot;
  uint32_t mask;
  int32_t max_keys;
  // per key slot
  int64_t* skey;
  int32_t* skg;
};

__device__ __forceinline__ uint32_t keymap_home(const KeyMap& m, int64_t key) {
  return (uint32_t)fmix64((uint64_t)key ^ 0x9E3779B97F4A7C15ull) & m.mask;
}
// the key's slot, or -1 (lookup only)
__device__ __forceinline__ int32_t keymap_find(const KeyMap& m, int64_t key) {
  uint32_t s = keymap_home(m, key);
  for (uint32_t probes = 0; probes <= m.mask; probes++) {
    if (m.mstate[s] == 0) return -1;
    if (m.mkey[s] == key) return (int32_t)m.mslot[s];
    s = (s + 1) & m.mask;
  }
  return -1;
}
// find or claim (the pattern of the count windows' key map): a claiming lane publishes key and slot before the state.
// nslots hands out the slots, map_full counts the refusals; a key that was refused a slot stays refused.
template <class KG>
__device__ __forceinline__ int32_t keymap_claim(const KeyMap& m, int32_t* nslots, unsigned long long* map_full,
                                                int64_t key, KG kg_of) {
  uint32_t s = keymap_home(m, key);
  for (uint32_t probes = 0; probes <= m.mask;) {
    const uint32_t cur = __hip_atomic_load(&m.mstate[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __atomic_signal_fence(__ATOMIC_ACQUIRE);
    if (cur == 2) {
      if (__hip_atomic_load(&m.mkey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == key) {
        const uint32_t slot = __hip_atomic_load(&m.mslot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (slot >= (uint32_t)m.max_keys) break;
        return (int32_t)slot;
      }
      s = (s + 1) & m.mask;
      probes++;
      continue;
    }
    if (cur == 1) continue;  // being published by another lane: re-read
    if (atomicCAS(&m.mstate[s], 0u, 1u) == 0u) {
      const int32_t slot = atomicAdd(nslots, 1);
      __hip_atomic_store(&m.mkey[s], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&m.mslot[s], (uint32_t)slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (slot < m.max_keys) {
        m.skey[slot] = key;
        m.skg[slot] = kg_of();
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(&m.mstate[s], 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (slot >= m.max_keys) {
        atomicAdd(map_full, 1ull);
        return -1;
      }
      return slot;
    }
  }
  atomicAdd(map_full, 1ull);
  return -1;
}
// rebuild of a grown map from the slots' keys (no lookups run beside it)
__global__ __launch_bounds__(256) void k_keymap_rehash(KeyMap m, int32_t nslots) {
  const int32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nslots) return;
  const int64_t key = m.skey[slot];
  uint32_t s = keymap_home(m, key);
  for (uint32_t probes = 0; probes <= m.mask; probes++) {
    if (atomicCAS(&m.mstate[s], 0u, 2u) == 0u) {
      m.mkey[s] = key;
      m.mslot[s] = (uint32_t)slot;
      return;
    }
    s = (s + 1) & m.mask;
  }
}

// ---------------------------------------------------------------- wave helpers
__device__ __forceinline__ unsigned long long wave_count(bool p) { return (unsigned long long)__popcll(__ballot(p)); }
__device__ __forceinline__ int64_t wave_min64(int64_t v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}

// ---------------------------------------------------------------- handle base
struct Buf {  // scratch that only grows; contents are not kept.  Owns its allocation.
  void* p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() {
    if (p) (void)hipFree(p);
  }
};

struct TableHandle {
  std::string err;
  bool ready = false;
  hipStream_t stream = nullptr;
  int device = 0;
  Buf b_tmp;  // rocprim's temporary storage, the drain's bounce buffer
  // pending output: n_out rows in columns of ocap rows; oseg: the (epoch, rows) segments they came in
  int64_t ocap = 0, n_out = 0;
  std::vector<std::pair<int64_t, int64_t>> oseg;
};

int set_err(TableHandle* op, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  op->err = buf;
  return code;
}
#define TB_HIP(op, expr)                                                                                   \
  do {                                                                                                     \
    hipError_t _e = (expr);                                                                                \
    if (_e != hipSuccess) return set_err(op, FW_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

inline unsigned grid_of(int64_t n, int t = 256) { return (unsigned)std::max<int64_t>(1, (n + t - 1) / t); }

int ensure(TableHandle* op, Buf& b, size_t bytes) {
  if (bytes <= b.cap) return FW_OK;
  size_t want = std::max(bytes, b.cap + b.cap / 2);
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  if (hipMalloc(&b.p, want) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    return set_err(op, FW_ERR_CAPACITY, "cannot allocate %zu bytes of scratch", want);
  }
  b.cap = want;
  return FW_OK;
}

template <class T>
int excl_scan(TableHandle* op, const T* in, T* out, int64_t n) {
  size_t bytes = 0;
  TB_HIP(op, rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), (size_t)n, rocprim::plus<T>(), op->stream));
  int rc = ensure(op, op->b_tmp, bytes);
  if (rc) return rc;
  TB_HIP(op, rocprim::exclusive_scan(op->b_tmp.p, bytes, in, out, T(0), (size_t)n, rocprim::plus<T>(), op->stream));
  return FW_OK;
}
// stable, on the keys' bits [0, end_bit)
template <class K>
int sort_pairs(TableHandle* op, const K* kin, K* kout, const uint32_t* vin, uint32_t* vout, int64_t n, unsigned end_bit) {
  size_t bytes = 0;
  TB_HIP(op, rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, (size_t)n, 0u, end_bit, op->stream));
  int rc = ensure(op, op->b_tmp, bytes);
  if (rc) return rc;
  TB_HIP(op, rocprim::radix_sort_pairs(op->b_tmp.p, bytes, kin, kout, vin, vout, (size_t)n, 0u, end_bit, op->stream));
  return FW_OK;
}

// the device counters to the host (settles the stream) and back; H: a handle with its counter struct at ctr (device)
// and hctr (pinned host copy)
template <class H>
int read_ctr(H* op) {
  TB_HIP(op, hipMemcpyAsync(op->hctr, op->ctr, sizeof(*op->ctr), hipMemcpyDeviceToHost, op->stream));
  TB_HIP(op, hipStreamSynchronize(op->stream));
  return FW_OK;
}
template <class H>
int write_ctr(H* op) {
  TB_HIP(op, hipMemcpyAsync(op->ctr, op->hctr, sizeof(*op->ctr), hipMemcpyHostToDevice, op->stream));
  TB_HIP(op, hipStreamSynchronize(op->stream));
  return FW_OK;
}

int settle(TableHandle* op) {
  TB_HIP(op, hipStreamSynchronize(op->stream));
  return FW_OK;
}

// ---------------------------------------------------------------- column sets
// One column of a store, a key map or the output: where its pointer lives, the bytes a row (or slot) takes in each of
// its `planes` (a column-major matrix has one plane of `cap` rows per column), and the byte fresh rows are filled
// with (-1: left as allocated).
struct Col {
  void** p;
  size_t w;
  int planes, fill;
};
template <class T>
Col col(T*& p, size_t w = sizeof(T), int planes = 1, int fill = -1) {
  return Col{(void**)&p, w, planes, fill};
}
using Cols = std::vector<Col>;

void cols_free(const Cols& cs) {
  for (const Col& c : cs) {
    (void)hipFree(*c.p);
    *c.p = nullptr;
  }
}
// `cap` rows for every column (the pointers come in null); false, and nothing allocated, when one does not fit
bool cols_alloc(const Cols& cs, int64_t cap) {
  for (const Col& c : cs)
    if (hipMalloc(c.p, (size_t)cap * c.w * c.planes) != hipSuccess) {
      (void)hipGetLastError();
      *c.p = nullptr;
      cols_free(cs);
      return false;
    }
  return true;
}
// the fill bytes, then the first n rows of `from` (the same columns at from_cap rows), queued on the handle's stream
int cols_init(TableHandle* op, const Cols& to, int64_t to_cap, const Cols& from, int64_t from_cap, int64_t n) {
  for (size_t q = 0; q < to.size(); q++) {
    const Col& c = to[q];
    if (c.fill >= 0) TB_HIP(op, hipMemsetAsync(*c.p, c.fill, (size_t)to_cap * c.w * c.planes, op->stream));
    for (int j = 0; n && j < c.planes; j++)
      TB_HIP(op, hipMemcpyAsync((char*)*c.p + (size_t)j * to_cap * c.w, (const char*)*from[q].p + (size_t)j * from_cap * c.w,
                                (size_t)n * c.w, hipMemcpyDeviceToDevice, op->stream));
  }
  return FW_OK;
}
// the capacity that holds `need`: from 1024, doubling
inline int64_t grown_cap(int64_t cap, int64_t need) {
  cap = std::max<int64_t>(cap, 1024);
  while (cap < need) cap *= 2;
  return cap;
}
// One set of columns to at least `need` rows, its first n rows kept.  S: the struct of pointers, cols_of(S&) its
// columns, cap its capacity; what: the refusal's text, with one %lld for the rows.
template <class S, class F>
int cols_grow(TableHandle* op, S& cur, int64_t& cap, int64_t need, int64_t n, F cols_of, const char* what) {
  if (need <= cap) return FW_OK;
  const int64_t ncap = grown_cap(cap, need);
  S next{};
  if (!cols_alloc(cols_of(next), ncap)) return set_err(op, FW_ERR_CAPACITY, what, (long long)ncap);
  int rc = cols_init(op, cols_of(next), ncap, cols_of(cur), cap, n);
  if (!rc && n) rc = settle(op);
  if (rc) {
    cols_free(cols_of(next));
    return rc;
  }
  cols_free(cols_of(cur));
  cur = next;
  cap = ncap;
  return FW_OK;
}
// Both buffers of a row store (R: the columns' pointers and `cap`) to at least `need` rows; the live one keeps its
// n rows and becomes buffer 0.
template <class R, class F>
int grow_store(TableHandle* op, R (&store)[2], int& cur, int64_t n, int64_t need, F cols_of) {
  if (need <= store[0].cap) return FW_OK;
  if (need >= (int64_t(1) << 31)) return set_err(op, FW_ERR_CAPACITY, "the row store would exceed 2^31 rows");
  const int64_t cap = grown_cap(store[0].cap, need);
  R a{}, b{};
  a.cap = b.cap = cap;
  if (!cols_alloc(cols_of(a), cap) || !cols_alloc(cols_of(b), cap)) {
    cols_free(cols_of(a));
    return set_err(op, FW_ERR_CAPACITY, "cannot allocate a row store of %lld rows", (long long)cap);
  }
  int rc = cols_init(op, cols_of(a), cap, cols_of(store[cur]), store[cur].cap, n);
  if (!rc && n) rc = settle(op);
  if (rc) {
    cols_free(cols_of(a));
    cols_free(cols_of(b));
    return rc;
  }
  cols_free(cols_of(store[0]));
  cols_free(cols_of(store[1]));
  store[0] = a;
  store[1] = b;
  cur = 0;
  return FW_OK;
}
// The key map's columns: the table's (2 * max_keys entries) and the slots' (max_keys: skey, skg, then own(m), the
// handle's own)
Cols keymap_table_cols(KeyMap& m) { return Cols{col(m.mkey), col(m.mstate, 4, 1, 0), col(m.mslot)}; }
template <class M, class F>
Cols keymap_slot_cols(M& m, F own) {
  Cols cs{col(m.skey), col(m.skg)};
  for (const Col& c : own(m)) cs.push_back(c);
  return cs;
}
template <class M, class F>
void free_map(M& map, F own) {
  cols_free(keymap_table_cols(map));
  cols_free(keymap_slot_cols(map, own));
  map = M{};
}
// A key map for at least `keys` keys, below 2^limit_bits; the slots' columns move over and the table is rebuilt from
// the slots' keys.
template <class M, class F>
int grow_map(TableHandle* op, M& map, int64_t nslots, int64_t keys, int limit_bits, F own) {
  if (keys <= map.max_keys) return FW_OK;
  if (keys >= (int64_t(1) << limit_bits)) return set_err(op, FW_ERR_CAPACITY, "the key map would exceed 2^%d keys", limit_bits);
  const int64_t mk = grown_cap(map.max_keys, keys), cap = mk * 2;
  M n{};
  n.mask = (uint32_t)(cap - 1);
  n.max_keys = (int32_t)mk;
  if (!cols_alloc(keymap_table_cols(n), cap) || !cols_alloc(keymap_slot_cols(n, own), mk)) {
    cols_free(keymap_table_cols(n));
    return set_err(op, FW_ERR_CAPACITY, "cannot allocate a key map of %lld keys", (long long)mk);
  }
  int rc = cols_init(op, keymap_table_cols(n), cap, keymap_table_cols(map), 0, 0);
  if (!rc) rc = cols_init(op, keymap_slot_cols(n, own), mk, keymap_slot_cols(map, own), map.max_keys, nslots);
  if (!rc && nslots)
    hipLaunchKernelGGL(k_keymap_rehash, dim3(grid_of(nslots)), dim3(256), 0, op->stream, (KeyMap)n, (int32_t)nslots);
  if (!rc) rc = settle(op);
  free_map(rc ? n : map, own);
  if (!rc) map = n;
  return rc;
}

// ---------------------------------------------------------------- pending output
// `rows` more pending rows of `epoch` (a call that adds to the last segment's epoch extends it)
void append_segment(TableHandle* op, int64_t epoch, int64_t rows) {
  if (rows == 0) return;
  if (!op->oseg.empty() && op->oseg.back().first == epoch) op->oseg.back().second += rows;
  else op->oseg.emplace_back(epoch, rows);
}
void clear_pending(TableHandle* op) {
  op->n_out = 0;
  op->oseg.clear();
}
struct DrainCol {  // a pending column: the caller's array (null: not wanted), the handle's, bytes per row
  void* dst;
  void* src;
  size_t w;
};
// the first min(cap, pending) rows to the caller, their epochs from the segment queue; the rest moves to the front
int drain_pending(TableHandle* op, const std::vector<DrainCol>& cols, int64_t* epoch, int64_t cap, int64_t* n) {
  const int64_t k = std::min(cap, op->n_out);
  *n = k;
  if (k == 0) return FW_OK;
  size_t wmax = 0;
  for (const DrainCol& c : cols) {
    wmax = std::max(wmax, c.w);
    if (c.dst) TB_HIP(op, hipMemcpyAsync(c.dst, c.src, (size_t)k * c.w, hipMemcpyDeviceToHost, op->stream));
  }
  const int64_t left = op->n_out - k;
  TB_HIP(op, hipStreamSynchronize(op->stream));
  if (left) {  // (a partial drain: the rest moves to the front through a bounce buffer)
    int rc;
    if ((rc = ensure(op, op->b_tmp, (size_t)left * wmax))) return rc;
    for (const DrainCol& c : cols) {
      TB_HIP(op, hipMemcpyAsync(op->b_tmp.p, (char*)c.src + (size_t)k * c.w, (size_t)left * c.w, hipMemcpyDeviceToDevice, op->stream));
      TB_HIP(op, hipMemcpyAsync(c.src, op->b_tmp.p, (size_t)left * c.w, hipMemcpyDeviceToDevice, op->stream));
    }
    TB_HIP(op, hipStreamSynchronize(op->stream));
  }
  int64_t w = 0;
  while (w < k && !op->oseg.empty()) {
    auto& s = op->oseg.front();
    const int64_t take = std::min(s.second, k - w);
    if (epoch) std::fill(epoch + w, epoch + w + take, s.first);
    w += take;
    s.second -= take;
    if (s.second == 0) op->oseg.erase(op->oseg.begin());
  }
  op->n_out = left;
  return FW_OK;
}

// ---------------------------------------------------------------- entry points
// The head of an entry point: a null handle, `bad` (an argument the call cannot do without), a handle that was not
// created.  The call's own argument checks follow, then on_device.
int enter(TableHandle* op, bool bad = false, const char* what = "null argument") {
  if (!op) return FW_ERR_ARG;
  if (bad) return set_err(op, FW_ERR_ARG, "%s", what);
  if (!op->ready) return set_err(op, FW_ERR_STATE, "the handle was not created");
  return FW_OK;
}
// ... of a snapshot or restore of key group kg; H: a handle whose config `c` has the KeyGroupRange as kg0, nkg
template <class H>
int enter_key_group(H* op, bool bad, const char* what, int32_t kg) {
  const int rc = enter(op, bad, what);
  if (rc) return rc;
  if (kg < op->c.kg0 || kg >= op->c.kg0 + op->c.nkg)
    return set_err(op, FW_ERR_KEY_GROUP, "key group %d outside KeyGroupRange [%d, %d]", kg, op->c.kg0, op->c.kg0 + op->c.nkg - 1);
  return FW_OK;
}
// ... of a push of n rows (null_column: a column it cannot do without is missing); H's config has key_kind
template <class H>
int enter_push(H* op, bool null_column, const int32_t* key_hash, int64_t n) {
  const int rc = enter(op);
  if (rc) return rc;
  if (n < 0 || (n > 0 && null_column)) return set_err(op, FW_ERR_ARG, "null column");
  if (op->c.key_kind == FW_KEY_HASHED && n > 0 && !key_hash)
    return set_err(op, FW_ERR_ARG, "key_hash required for FW_KEY_HASHED");
  return FW_OK;
}
int on_device(TableHandle* op) {
  TB_HIP(op, hipSetDevice(op->device));
  return FW_OK;
}

// A restore's checks of the keys: every row count >= 0 (then per_key(i), the handle's own check of key i), the key in
// key group kg, the counts' total n_rows.  C: the handle's config (key_kind, max_par).
template <class C, class F>
int check_restored_keys(TableHandle* op, const C& c, int32_t kg, const int64_t* key, const int64_t* rows_of,
                        int64_t n_keys, int64_t n_rows, F per_key) {
  int64_t total = 0;
  for (int64_t i = 0; i < n_keys; i++) {
    if (rows_of[i] < 0) return set_err(op, FW_ERR_ARG, "negative n_rows");
    const int rc = per_key(i);
    if (rc) return rc;
    total += rows_of[i];
    if (c.key_kind != FW_KEY_HASHED && host_key_group(host_key_hash(key[i], c.key_kind == FW_KEY_INT), c.max_par) != kg)
      return set_err(op, FW_ERR_KEY_GROUP, "key %lld is not in key group %d", (long long)key[i], kg);
  }
  if (total != n_rows) return set_err(op, FW_ERR_ARG, "n_rows does not match the keys' row counts");
  return FW_OK;
}
// ... and no key twice; `seen` takes the keys, for the handle's own "already has state" check
int check_restored_unique(TableHandle* op, const int64_t* key, int64_t n_keys, std::unordered_set<int64_t>& seen) {
  for (int64_t i = 0; i < n_keys; i++)
    if (!seen.insert(key[i]).second)
      return set_err(op, FW_ERR_STATE, "key %lld occurs twice in the restored state", (long long)key[i]);
  return FW_OK;
}

}  // namespace
