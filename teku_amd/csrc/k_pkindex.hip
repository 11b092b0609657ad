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
#include "tb_pkcomb.h"

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
//
// REF (k_pk_lookup_ref, a device with comb rows: tb_pkcomb.h):
// pk_ref[i] = key i's reference word -- the table's row when tab_comb_on (the
// table has a comb region) and its code is TB_SUCCESS, the cache's row when it
// lies below comb_cap and its ready byte is set, else TB_PKREF_NONE (a miss
// too).  The ready bytes were set by k_pk_learn_comb of earlier launches, which
// this one is ordered behind as it is behind their rows (tb_lib.hip
// launch_partial): no launch reads a comb row that its own batch builds.
template <bool REF>
__device__ TB_INLINE void pk_lookup_body(const uint8_t* __restrict__ pks, uint32_t K, uint32_t align, const uint32_t* __restrict__ slots, uint32_t mask,
                                         uint64_t seed, const uint32_t* __restrict__ tab_keys, const g1a* __restrict__ tab_aff,
                                         const uint8_t* __restrict__ tab_code, const pkx_cache& cache, g1a* __restrict__ pk_aff,
                                         uint8_t* __restrict__ pk_code, uint32_t* __restrict__ miss, unsigned long long* __restrict__ stat,
                                         uint32_t* __restrict__ pk_ref, const uint8_t* __restrict__ cache_ready, uint32_t comb_cap,
                                         uint32_t tab_comb_on) {
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
    const uint8_t code = tab_hit ? tab_code[h.idx] : (uint8_t)TB_SUCCESS;
    pk_code[i] = code;
    if (REF)
      pk_ref[i] = tab_hit ? comb_ref(true, h.idx, tab_comb_on && code == TB_SUCCESS)
                          : comb_ref(false, h.idx, comb_row_in_cap(h.idx, comb_cap) && cache_ready[h.idx] != 0);
  } else if (REF && live) {
    pk_ref[i] = TB_PKREF_NONE;
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

extern "C" __global__ void __launch_bounds__(TB_PKX_BLOCK)
    k_pk_lookup(const uint8_t* __restrict__ pks, uint32_t K, uint32_t align, const uint32_t* __restrict__ slots, uint32_t mask, uint64_t seed,
                const uint32_t* __restrict__ tab_keys, const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, pkx_cache cache,
                g1a* __restrict__ pk_aff, uint8_t* __restrict__ pk_code, uint32_t* __restrict__ miss, unsigned long long* __restrict__ stat) {
  pk_lookup_body<false>(pks, K, align, slots, mask, seed, tab_keys, tab_aff, tab_code, cache, pk_aff, pk_code, miss, stat, nullptr, nullptr, 0u, 0u);
}

extern "C" __global__ void __launch_bounds__(TB_PKX_BLOCK)
    k_pk_lookup_ref(const uint8_t* __restrict__ pks, uint32_t K, uint32_t align, const uint32_t* __restrict__ slots, uint32_t mask, uint64_t seed,
                    const uint32_t* __restrict__ tab_keys, const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, pkx_cache cache,
                    g1a* __restrict__ pk_aff, uint8_t* __restrict__ pk_code, uint32_t* __restrict__ miss, unsigned long long* __restrict__ stat,
                    uint32_t* __restrict__ pk_ref, const uint8_t* __restrict__ cache_ready, uint32_t comb_cap, uint32_t tab_comb_on) {
  pk_lookup_body<true>(pks, K, align, slots, mask, seed, tab_keys, tab_aff, tab_code, cache, pk_aff, pk_code, miss, stat, pk_ref, cache_ready, comb_cap,
                       tab_comb_on);
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

// comb_build's working memory on the device: a column of LDS per lane
// (TB_PKCOMB_TMP x 48 B x TB_PKCOMB_BLOCK lanes = 43,008 B per workgroup).
struct comb_lds {
  fp z[TB_PKCOMB_TMP][TB_PKCOMB_BLOCK];
};

// k_pk_learn on a device whose cache has a comb region (tb_pkcomb.h, DESIGN.md
// 3n): the same append, and for a key whose append published a row below
// comb_cap the row's 15 comb entries (comb_build) and then its ready byte.
// TB_PKX_DUP, TB_PKX_FULL and TB_PKX_MISS get no comb row: the one appender
// that published the bytes builds it.  It takes k_pk_learn's place on the key
// stream, behind the join and ahead of the record of e_learn, so whatever
// orders a later launch's lookup behind this batch's rows orders it behind
// their comb entries and ready bytes too; nothing of this batch reads them
// (its references were written by its own lookup, before this kernel).  The
// ready byte is a plain store behind the entries' stores: readers are later
// launches.  Workgroups of TB_PKCOMB_BLOCK threads walk the miss list with the
// grid's stride (the host bounds the grid: the list's length is only known
// here).  comb_stat[1] += the rows built.
extern "C" __global__ void __launch_bounds__(TB_PKCOMB_BLOCK)
    k_pk_learn_comb(const uint8_t* __restrict__ pks, uint32_t align, const uint32_t* __restrict__ list, const g1a* __restrict__ pk_aff,
                    const uint8_t* __restrict__ pk_code, pkx_cache cache, g1a* __restrict__ cache_comb, uint8_t* __restrict__ cache_ready,
                    uint32_t comb_cap, unsigned long long* __restrict__ comb_stat) {
  __shared__ comb_lds lds;
  const uint32_t count = list[0];
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) {
    const uint32_t i = list[1u + t];
    if (pk_code[i] != TB_SUCCESS) continue;
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
    const uint32_t row = pkx_append(cache, q, pt);
    if (row >= cache.rows || !comb_row_in_cap(row, comb_cap)) continue;  // TB_PKX_DUP / FULL / MISS, or beyond the cap
    comb_build(cache_comb + (size_t)row * TB_PKCOMB_ENTRIES, pk_aff[i], &lds.z[0][threadIdx.x], TB_PKCOMB_BLOCK);
    comb_mark_ready(cache_ready, row, comb_cap);
    atomicAdd(comb_stat + 1, 1ull);
  }
}

// tbls_pk_table_load: the comb rows of the table's K keys, row i for key i;
// a key whose code is not TB_SUCCESS gets none (its row is never read: the key
// stage fails its sets first).  comb_stat[2] += the rows built.
extern "C" __global__ void __launch_bounds__(TB_PKCOMB_BLOCK)
    k_pk_comb_build(const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, uint32_t K, g1a* __restrict__ tab_comb,
                    unsigned long long* __restrict__ comb_stat) {
  __shared__ comb_lds lds;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < K; i += gridDim.x * blockDim.x) {
    if (tab_code[i] != TB_SUCCESS) continue;
    comb_build(tab_comb + (size_t)i * TB_PKCOMB_ENTRIES, tab_aff[i], &lds.z[0][threadIdx.x], TB_PKCOMB_BLOCK);
    atomicAdd(comb_stat + 2, 1ull);
  }
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
