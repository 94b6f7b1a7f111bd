// fw_keygroup.h — KeyGroupRangeAssignment.computeKeyGroupForKeyHash on the host: MathUtils.murmurHash(hash) %
// maxParallelism (MathUtils.java:134-154).  The operators' restore paths check restored keys with it before anything
// changes; the device's is fw_jmath.h key_group.
#pragma once
#include <cstdint>

// hashCode of a Long (the halves folded, Long.hashCode) or Integer key
inline int32_t host_key_hash(int64_t key, bool int_key) {
  return int_key ? (int32_t)key : (int32_t)(key ^ (int64_t)((uint64_t)key >> 32));
}
inline int32_t host_key_group(int32_t hash, int32_t max_par) {
  uint32_t c = (uint32_t)hash;
  c *= 0xcc9e2d51u;
  c = (c << 15) | (c >> 17);
  c *= 0x1b873593u;
  c = (c << 13) | (c >> 19);
  c = c * 5u + 0xe6546b64u;
  c ^= 4u;
  c ^= c >> 16;
  c *= 0x85ebca6bu;
  c ^= c >> 13;
  c *= 0xc2b2ae35u;
  c ^= c >> 16;
  const int32_t r = (int32_t)c;
  return (r >= 0 ? r : (r != INT32_MIN ? -r : 0)) % max_par;
}
