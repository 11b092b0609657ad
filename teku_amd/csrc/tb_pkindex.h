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

// ---------------------------------------------------------------------------
// The learned key cache: an index of the same kind that grows
// while batches run.  A row is a key's 48 bytes and the 96-byte affine point
// the key stage computed from them; rows are only ever appended, and a slot is
// published after its row, so a reader that sees a slot sees its row.
//
//  * an appender probes like a lookup; at the first empty slot it reserves a
//    row (one atomic add on the row counter), writes the row, makes it visible
//    (pkx_release) and publishes the slot with a compare-and-swap.  When the
//    swap loses to another key it keeps its row and probes on; when it loses to
//    equal bytes (two sets of one batch carry the same key) it stops: the
//    bytes have one findable entry and the reserved row stays unused;
//  * an appender that reads a slot another appender of the same launch
//    published reads the row behind an acquire (pkx_acquire); lookups run in
//    later launches and need none;
//  * when no row is left the key is refused (TB_PKX_FULL) and counted: nothing
//    is evicted; `rows` is fixed and `mask + 1` is pkx_capacity(rows), so the
//    load factor stays at most 1/2.
//
// tests/native/pkcache_check.cpp runs these on the CPU.
#define TB_PKX_POINT_WORDS 24u   // a 96-byte affine point
#define TB_PKX_DUP 0xfffffffeu   // pkx_append: equal bytes are in the cache already
#define TB_PKX_FULL 0xfffffffdu  // pkx_append: no row left
enum { TB_PKC_HITS = 0, TB_PKC_LEARNED = 1, TB_PKC_REFUSED = 2, TB_PKC_STATS = 3 };  // pkx_cache::stat

struct pkx_cache {
  uint32_t* slots;  // mask + 1 of them (nullptr: no cache)
  uint32_t mask;
  uint32_t* keys;    // rows x 12 words
  uint32_t* points;  // rows x 24 words
  uint32_t rows;
  uint32_t* n_rows;  // rows reserved; concurrent appenders may push it a little past `rows`
  unsigned long long* stat;  // TB_PKC_*: lookups' hits, rows published, keys refused for want of a row
  uint64_t seed;
};

TB_HD TB_INLINE uint32_t pkx_word_load(const uint32_t* p) {
#if TB_DEVICE_PASS
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

// Between the row's stores and the slot's compare-and-swap: the stores reach
// memory every compute die reads (an agent-scope release; the explicit wait
// keeps the swap behind the write-back).
TB_HD TB_INLINE void pkx_release() {
#if TB_DEVICE_PASS
  __threadfence();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}

// Between reading a slot and reading its row within one launch: drops this
// compute unit's cached lines (an agent-scope acquire).
TB_HD TB_INLINE void pkx_acquire() {
#if TB_DEVICE_PASS
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
}

TB_HD TB_INLINE void pkx_count(unsigned long long* p) {
#if TB_DEVICE_PASS
  atomicAdd(p, 1ull);
#else
  ++*p;
#endif
}

// A free row's index, or TB_PKX_MISS when every row is taken.
TB_HD TB_INLINE uint32_t pkx_reserve(const pkx_cache& c) {
  if (pkx_word_load(c.n_rows) >= c.rows) return TB_PKX_MISS;  // a full cache's counter stops growing
#if TB_DEVICE_PASS
  const uint32_t r = atomicAdd(c.n_rows, 1u);
#else
  const uint32_t r = (*c.n_rows)++;
#endif
  return r < c.rows ? r : TB_PKX_MISS;
}

// Append the key q with its point pt.  Returns the row it published;
// TB_PKX_DUP when equal bytes are in the cache (before, or by a concurrent
// appender); TB_PKX_FULL when no row is left; TB_PKX_MISS when no slot was
// free within the probe bound.
TB_HD TB_INLINE uint32_t pkx_append(const pkx_cache& c, const uint32_t q[TB_PKX_WORDS], const uint32_t pt[TB_PKX_POINT_WORDS]) {
  uint32_t s = pkx_first(pkx_hash(q, c.seed), c.mask);
  const uint32_t bound = pkx_probe_bound(c.mask + 1u);
  uint32_t row = TB_PKX_MISS;
  for (uint32_t p = 0; p < bound; p++, s = pkx_next(s, c.mask)) {
    uint32_t v = pkx_word_load(c.slots + s);
    if (v == 0) {
      if (row == TB_PKX_MISS) {
        row = pkx_reserve(c);
        if (row == TB_PKX_MISS) {
          pkx_count(c.stat + TB_PKC_REFUSED);
          return TB_PKX_FULL;
        }
        uint32_t* k = c.keys + (size_t)row * TB_PKX_WORDS;
        uint32_t* a = c.points + (size_t)row * TB_PKX_POINT_WORDS;
        TB_UNROLL for (uint32_t i = 0; i < TB_PKX_WORDS; i++) k[i] = q[i];
        TB_UNROLL for (uint32_t i = 0; i < TB_PKX_POINT_WORDS; i++) a[i] = pt[i];
        pkx_release();
      }
      v = pkx_cas(c.slots + s, 0u, row + 1u);
      if (v == 0) {
        pkx_count(c.stat + TB_PKC_LEARNED);
        return row;
      }
    }
    pkx_acquire();
    if (pkx_equal(c.keys + (size_t)(v - 1u) * TB_PKX_WORDS, q)) return TB_PKX_DUP;
  }
  return TB_PKX_MISS;
}

// The key stage's lookup of the key q: the loaded table's index first
// (t_slots, nullptr: no table), then the cache (c.slots, nullptr: none).
#define TB_PKX_SRC_NONE 0u
#define TB_PKX_SRC_TABLE 1u
#define TB_PKX_SRC_CACHE 2u
struct pkx_hit {
  uint32_t src, idx;  // TB_PKX_SRC_*; the table index or the cache row (TB_PKX_MISS with TB_PKX_SRC_NONE)
};
TB_HD TB_INLINE pkx_hit pkx_find_two(const uint32_t* t_slots, uint32_t t_mask, const uint32_t* t_keys, uint64_t t_seed, const pkx_cache& c,
                                     const uint32_t q[TB_PKX_WORDS]) {
  uint32_t i = t_slots ? pkx_find(t_slots, t_mask, t_keys, q, t_seed) : TB_PKX_MISS;
  if (i != TB_PKX_MISS) return {TB_PKX_SRC_TABLE, i};
  i = c.slots ? pkx_find(c.slots, c.mask, c.keys, q, c.seed) : TB_PKX_MISS;
  if (i != TB_PKX_MISS) return {TB_PKX_SRC_CACHE, i};
  return {TB_PKX_SRC_NONE, TB_PKX_MISS};
}

}  // namespace tb
