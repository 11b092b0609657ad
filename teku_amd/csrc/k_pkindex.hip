// The key table's index over its compressed key bytes (tb_pkindex.h): built at
// tbls_pk_table_load, probed by the key stage of batches that name keys by
// their bytes, and by tbls_pk_table_resolve; and the learned key cache behind
// it (tb_pkindex.h pkx_cache), which the same key stages probe after the
// table and extend with the valid keys they had to decompress (k_pk_learn).
//
// The lookup is a latency-bound gather (a 48-byte read, a hash, one or two
// dependent slot reads, a 48-byte compare and a 97-byte copy per key; the
// probing is pkx_find, the function the CPU check runs), so it runs 256-thread
// workgroups with few registers: many waves per SIMD hide the dependent
// loads.  The keys it does not find go to a compacted list, so that
// the square-root and subgroup-check chains of k_pk_decompress_list run in
// full waves of unknown keys instead of in the one lane per wave that missed.
#include "tb_kdecl.h"
#include "tb_pkindex.h"

using namespace tb;

static_assert(sizeof(g1a) == 96, "a table entry is copied as six 16-byte words");
static_assert(sizeof(g1a) == 4 * TB_PKX_POINT_WORDS, "a cache row's point is a g1a");

#define TB_PKX_BLOCK 256

// One thread per table key inserts it (atomicCAS, linear probing).  slots is
// zeroed by the host.
extern "C" __global__ void __launch_bounds__(TB_PKX_BLOCK)
    k_pkx_build(const uint32_t* __restrict__ keys, uint32_t K, uint32_t* slots, uint32_t mask, uint64_t seed) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  (void)pkx_insert(slots, mask, keys, i, seed);
}

// The 12 words of key i of pks: 16-byte loads when the base allows them (the
// library's staging; the table's own keys), else 4-byte loads, else bytes (a
// caller's tbls_dev_batch.pks may sit anywhere).  align: the base's alignment,
// 16, 4 or 1 (wave-uniform).
__device__ TB_INLINE void pkx_load_key(uint32_t q[TB_PKX_WORDS], const uint8_t* __restrict__ pks, uint32_t i, uint32_t align) {
  const uint8_t* b = pks + (size_t)i * 48;
  if (align == 16) {
    const uint4* v = reinterpret_cast<const uint4*>(b);
    TB_UNROLL for (int k = 0; k < 3; k++) {
      const uint4 t = v[k];
      q[4 * k] = t.x;
      q[4 * k + 1] = t.y;
      q[4 * k + 2] = t.z;
      q[4 * k + 3] = t.w;
    }
  } else if (align == 4) {
    const uint32_t* v = reinterpret_cast<const uint32_t*>(b);
    TB_UNROLL for (int k = 0; k < 12; k++) q[k] = v[k];
  } else {
    TB_UNROLL for (int k = 0; k < 12; k++)
      q[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
  }
}

// The key stage's lookup, one thread per key of the batch: the loaded table's
// index first (slots, nullptr: no table), then the learned cache (cache.slots,
// nullptr: none) -- pkx_find_two.  A hit copies the affine point and status to
// pk_aff[i] / pk_code[i]: the table's entry, or the cache row's point with
// TB_SUCCESS (only valid keys are learned); either holds what stage_pk wrote
// for the same 48 bytes.  A miss appends i to miss[1 ..) -- miss[0] is the
// count, zeroed by the host -- with one atomicAdd per wave.  With a table,
// stat[0] += its hits and stat[1] += its misses (cache hits among them);
// cache.stat[TB_PKC_HITS] += the cache's hits; one 64-bit atomic each per wave.
extern "C" __global__ void __launch_bounds__(TB_PKX_BLOCK)
    k_pk_lookup(const uint8_t* __restrict__ pks, uint32_t K, uint32_t align, const uint32_t* __restrict__ slots, uint32_t mask, uint64_t seed,
                const uint32_t* __restrict__ tab_keys, const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, pkx_cache cache,
                g1a* __restrict__ pk_aff, uint8_t* __restrict__ pk_code, uint32_t* __restrict__ miss, unsigned long long* __restrict__ stat) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < K;
  pkx_hit h = {TB_PKX_SRC_NONE, TB_PKX_MISS};
  if (live) {
    uint32_t q[TB_PKX_WORDS];
    pkx_load_key(q, pks, i, align);
    h = pkx_find_two(slots, mask, tab_keys, seed, cache, q);
  }
  const bool tab_hit = h.src == TB_PKX_SRC_TABLE, cache_hit = h.src == TB_PKX_SRC_CACHE, lost = live && h.src == TB_PKX_SRC_NONE;
  if (tab_hit || cache_hit) {
    const uint4* src = tab_hit ? reinterpret_cast<const uint4*>(tab_aff + h.idx)
                               : reinterpret_cast<const uint4*>(cache.points + (size_t)h.idx * TB_PKX_POINT_WORDS);
    uint4* dst = reinterpret_cast<uint4*>(pk_aff + i);
    uint4 t[6];
    TB_UNROLL for (int k = 0; k < 6; k++) t[k] = src[k];
    TB_UNROLL for (int k = 0; k < 6; k++) dst[k] = t[k];
    pk_code[i] = tab_hit ? tab_code[h.idx] : (uint8_t)TB_SUCCESS;
  }
  // every lane of the wave is here (no early return above)
  const unsigned long long mh = __ballot(tab_hit), mc = __ballot(cache_hit), mm = __ballot(lost);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nh = (uint32_t)__popcll(mh), nc = (uint32_t)__popcll(mc), nm = (uint32_t)__popcll(mm);
  uint32_t base = 0;
  if (lane == 0) {
    if (nm) base = atomicAdd(miss, nm);
    if (slots) {
      if (nh) atomicAdd(stat, (unsigned long long)nh);
      if (nc + nm) atomicAdd(stat + 1, (unsigned long long)(nc + nm));
    }
    if (nc) atomicAdd(cache.stat + TB_PKC_HITS, (unsigned long long)nc);
  }
  base = __shfl(base, 0);
  if (lost) miss[1u + base + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull))] = i;
}

// k_pk_decompress over the compacted misses: list[0] keys list[1 ..).  The
// grid covers the batch's key count (the list's length is only known on the
// device); threads past the count return at once.  seen (nullable): a word of
// pinned host memory that takes the count, for the host's guess at the next
// batch (tb_lib.hip pk_keys_known) -- a plain store; nothing waits for it.
extern "C" __global__ void __launch_bounds__(TB_BLOCK, 2)
    k_pk_decompress_list(const uint8_t* __restrict__ pks, const uint32_t* __restrict__ list, g1a* __restrict__ pk_aff,
                         uint8_t* __restrict__ pk_code, uint32_t* __restrict__ seen) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0 && seen) *seen = list[0];
  if (t >= list[0]) return;
  const uint32_t i = list[1u + t];
  g1a a;
  const int code = stage_pk(pks + (size_t)i * 48, a);
  pk_aff[i] = a;
  pk_code[i] = (uint8_t)code;
}

// The end of the key stage with a learned cache: the keys of the miss list
// that k_pk_decompress_list found valid (pk_code TB_SUCCESS) are appended to
// the cache with the points it wrote (pkx_append; the infinity key and invalid
// keys are decoded every time).  The grid covers the batch's key count, as
// k_pk_decompress_list's; 256-thread workgroups, as the lookup's.
extern "C" __global__ void __launch_bounds__(TB_PKX_BLOCK)
    k_pk_learn(const uint8_t* __restrict__ pks, uint32_t align, const uint32_t* __restrict__ list, const g1a* __restrict__ pk_aff,
               const uint8_t* __restrict__ pk_code, pkx_cache cache) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= list[0]) return;
  const uint32_t i = list[1u + t];
  if (pk_code[i] != TB_SUCCESS) return;
  uint32_t q[TB_PKX_WORDS], pt[TB_PKX_POINT_WORDS];
  pkx_load_key(q, pks, i, align);
  const uint4* src = reinterpret_cast<const uint4*>(pk_aff + i);
  TB_UNROLL for (int k = 0; k < 6; k++) {
    const uint4 v = src[k];
    pt[4 * k] = v.x;
    pt[4 * k + 1] = v.y;
    pt[4 * k + 2] = v.z;
    pt[4 * k + 3] = v.w;
  }
  (void)pkx_append(cache, q, pt);
}

// tbls_pk_table_resolve: idx_out[i] = a table index whose bytes equal key i's,
// or TB_PKX_MISS.
extern "C" __global__ void __launch_bounds__(TB_PKX_BLOCK)
    k_pk_resolve(const uint8_t* __restrict__ pks, uint32_t n, uint32_t align, const uint32_t* __restrict__ slots, uint32_t mask, uint64_t seed,
                 const uint32_t* __restrict__ tab_keys, uint32_t* __restrict__ idx_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t q[TB_PKX_WORDS];
  pkx_load_key(q, pks, i, align);
  idx_out[i] = pkx_find(slots, mask, tab_keys, q, seed);
}
