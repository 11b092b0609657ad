// The key table's index over its compressed key bytes: an open-addressing
// hash table that maps the 48 bytes of a key to its table index, so a batch
// that names keys by their bytes finds the table's decompressed point
// (k_pkindex.hip, tbls_pk_table_load / tbls_pk_table_resolve).
//
//  * slots are 32-bit: index + 1, 0 = empty; the capacity is a power of two of
//    at least 2 K (pkx_capacity), so the load factor is at most 1/2;
//  * a key is 12 words as they lie in memory; its first slot is a keyed hash
//    of them (SipHash-1-3, the key derived from a 64-bit seed drawn at every
//    table load): validator keys are chosen by depositors, who could grind
//    keys into one long chain of an unkeyed hash;
//  * linear probing, at most pkx_probe_bound(capacity) slots: a lookup that
//    reaches the bound, or an empty slot, is a miss; a key that finds no free
//    slot within the bound stays out of the index.  A miss is always safe (the
//    caller decompresses the key); a hit is equality of all 48 bytes, never
//    of a fingerprint;
//  * a key whose bytes equal an inserted key's is not inserted again (either
//    index names the same bytes).
//
// Host and device run the same functions: the product builds and probes the
// index on the device only; tests/native/pkindex_check.cpp runs them on the CPU.
#pragma once
#include "tb_common.h"

#ifndef TB_PKX_PROBE_MAX
#define TB_PKX_PROBE_MAX 64u  // slots a lookup or an insertion visits at most
#endif
#define TB_PKX_WORDS 12u            // a 48-byte key
#define TB_PKX_MISS 0xffffffffu     // no index (tbls_pk_table_resolve's answer for an unknown key)

namespace tb {

// Smallest power of two >= 2 K, at least 8 (K <= 2^30).
TB_HD TB_INLINE uint32_t pkx_capacity(uint32_t K) {
  uint32_t c = 8;
  while (c < 2u * K && c < 0x80000000u) c <<= 1;
  return c;
}

TB_HD TB_INLINE uint32_t pkx_probe_bound(uint32_t cap) { return cap < TB_PKX_PROBE_MAX ? cap : TB_PKX_PROBE_MAX; }

TB_HD TB_INLINE uint64_t pkx_rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

#define TB_PKX_SIPROUND          \
  do {                           \
    v0 += v1;                    \
    v1 = pkx_rotl(v1, 13) ^ v0;  \
    v0 = pkx_rotl(v0, 32);       \
    v2 += v3;                    \
    v3 = pkx_rotl(v3, 16) ^ v2;  \
    v0 += v3;                    \
    v3 = pkx_rotl(v3, 21) ^ v0;  \
    v2 += v1;                    \
    v1 = pkx_rotl(v1, 17) ^ v2;  \
    v2 = pkx_rotl(v2, 32);       \
  } while (0)

// SipHash-1-3 of the 12 key words (as 6 little-endian 64-bit words); k0 = seed,
// k1 = a fixed bijection of it (splitmix64's finalizer).
TB_HD TB_INLINE uint64_t pkx_hash(const uint32_t w[TB_PKX_WORDS], uint64_t seed) {
  uint64_t k1 = seed + 0x9e3779b97f4a7c15ull;
  k1 = (k1 ^ (k1 >> 30)) * 0xbf58476d1ce4e5b9ull;
  k1 = (k1 ^ (k1 >> 27)) * 0x94d049bb133111ebull;
  k1 ^= k1 >> 31;
  uint64_t v0 = 0x736f6d6570736575ull ^ seed, v1 = 0x646f72616e646f6dull ^ k1, v2 = 0x6c7967656e657261ull ^ seed, v3 = 0x7465646279746573ull ^ k1;
  TB_UNROLL for (int i = 0; i < 6; i++) {
    const uint64_t m = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    v3 ^= m;
    TB_PKX_SIPROUND;
    v0 ^= m;
  }
  const uint64_t b = 48ull << 56;  // the length block
  v3 ^= b;
  TB_PKX_SIPROUND;
  v0 ^= b;
  v2 ^= 0xff;
  TB_PKX_SIPROUND;
  TB_PKX_SIPROUND;
  TB_PKX_SIPROUND;
  return v0 ^ v1 ^ v2 ^ v3;
}
#undef TB_PKX_SIPROUND

// The probe sequence: the first slot of a hash, and the slot after a slot
// (mask = capacity - 1; the sequence wraps past the last slot).
TB_HD TB_INLINE uint32_t pkx_first(uint64_t h, uint32_t mask) { return (uint32_t)(h ^ (h >> 32)) & mask; }
TB_HD TB_INLINE uint32_t pkx_next(uint32_t slot, uint32_t mask) { return (slot + 1u) & mask; }

TB_HD TB_INLINE bool pkx_equal(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
  TB_UNROLL for (uint32_t i = 0; i < TB_PKX_WORDS; i++) d |= a[i] ^ b[i];
  return d == 0;
}

// The table index of the key q (12 words), or TB_PKX_MISS.  slots: the index
// (capacity mask + 1), keys: the table's keys, 12 words each, 16-byte aligned
// (a device allocation; the compare then takes three 16-byte loads).  The
// index is complete and read-only while lookups run.
TB_HD TB_INLINE uint32_t pkx_find(const uint32_t* slots, uint32_t mask, const uint32_t* keys_, const uint32_t q[TB_PKX_WORDS], uint64_t seed) {
  const uint32_t* keys = static_cast<const uint32_t*>(__builtin_assume_aligned(keys_, 16));
  uint32_t s = pkx_first(pkx_hash(q, seed), mask);
  const uint32_t bound = pkx_probe_bound(mask + 1u);
  for (uint32_t p = 0; p < bound; p++, s = pkx_next(s, mask)) {
    const uint32_t v = slots[s];
    if (v == 0) return TB_PKX_MISS;
    if (pkx_equal(keys + (size_t)(v - 1u) * TB_PKX_WORDS, q)) return v - 1u;
  }
  return TB_PKX_MISS;
}

// Compare-and-swap of a slot: the device's atomicCAS (one thread per key
// inserts), a plain one on the host.  Returns the slot's previous value.
TB_HD TB_INLINE uint32_t pkx_cas(uint32_t* slot, uint32_t expect, uint32_t val) {
#if TB_DEVICE_PASS
  return atomicCAS(slot, expect, val);
#else
  const uint32_t old = *slot;
  if (old == expect) *slot = val;
  return old;
#endif
}

// Insert table key i.  Returns the slot it took, or TB_PKX_MISS when an equal
// key was there already or no slot was free within the probe bound.  Every
// inserter of equal bytes walks the same slots and slots never empty, so of
// concurrent equal keys exactly one is inserted.
TB_HD TB_INLINE uint32_t pkx_insert(uint32_t* slots, uint32_t mask, const uint32_t* keys, uint32_t i, uint64_t seed) {
  const uint32_t* q = keys + (size_t)i * TB_PKX_WORDS;
  uint32_t s = pkx_first(pkx_hash(q, seed), mask);
  const uint32_t bound = pkx_probe_bound(mask + 1u);
  for (uint32_t p = 0; p < bound; p++, s = pkx_next(s, mask)) {
#if TB_DEVICE_PASS
    uint32_t v = __atomic_load_n(slots + s, __ATOMIC_RELAXED);
#else
    uint32_t v = slots[s];
#endif
    if (v == 0) {
      v = pkx_cas(slots + s, 0u, i + 1u);
      if (v == 0) return s;
    }
    if (pkx_equal(keys + (size_t)(v - 1u) * TB_PKX_WORDS, q)) return TB_PKX_MISS;
  }
  return TB_PKX_MISS;
}

}  // namespace tb
