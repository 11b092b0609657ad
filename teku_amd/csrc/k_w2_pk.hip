// k_set_pk at two waves per SIMD (see k_w2_hash.hip for why a translation unit
// of its own): per set, aggregate key and P = [r] apk (affine).
#include "tb_kbody.h"
#include "tb_pkcomb.h"

using namespace tb;

namespace {
// g1_mul_u64_aff_w2 (tb_curve.h) with its window table {P, 2P, 3P} parked in
// the lane's LDS slots (tab[0], tab[TB_BLOCK], tab[2 TB_BLOCK]): each window
// reads its digit's entry instead of selecting among three register-resident
// points, which at 256 registers spilled the loop state every window.  Same
// chain, same result.
__device__ TB_INLINE g1j mul_u64_aff_w2_lds(const g1a& P, uint64_t k, g1a* tab) {
  const g1j P2j = jac_dbl_i(jac_from_aff(P));
  const g1j P3j = jac_add_aff_i(P2j, P);
  const fp zz = fp_mul(P2j.z, P3j.z);
  const fp iz = fp_inv(zz);
  const fp i2 = fp_mul(iz, P3j.z), i3 = fp_mul(iz, P2j.z);
  const fp i22 = fp_sqr(i2), i33 = fp_sqr(i3);
  tab[0] = P;
  tab[TB_BLOCK] = g1a{fp_mul(P2j.x, i22), fp_mul(fp_mul(P2j.y, i22), i2)};
  tab[2 * TB_BLOCK] = g1a{fp_mul(P3j.x, i33), fp_mul(fp_mul(P3j.y, i33), i3)};
  asm volatile("" ::: "memory");
  const int top = 63 - __builtin_clzll(k);
  int w = top >> 1;
  uint32_t d = (uint32_t)(k >> (2 * w)) & 3u;  // != 0
  g1j r = jac_from_aff(tab[(d - 1) * TB_BLOCK]);
  TB_NOUNROLL for (--w; w >= 0; --w) {
    r = jac_dbl_i(jac_dbl_i(r));
    d = (uint32_t)(k >> (2 * w)) & 3u;
    if (d) r = jac_add_aff_i(r, tab[(d - 1) * TB_BLOCK]);
  }
  return r;
}
}  // namespace

extern "C" __global__ void __launch_bounds__(TB_BLOCK, 2)
    k_set_pk_w2(const uint32_t* __restrict__ pk_off, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code,
                const uint64_t* __restrict__ rand, uint32_t n, g1a* __restrict__ P, uint8_t* __restrict__ set_code,
                uint32_t* __restrict__ n_bad, const uint32_t* __restrict__ key_idx, uint32_t tab_n, uint32_t multi_wave,
                g1a* __restrict__ P2, const g1a* __restrict__ comb) {
  __shared__ g1a tab[3 * TB_BLOCK];  // 288 B per lane: 147 KB per CU at two waves per SIMD
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = pk_off[i], e = pk_off[i + 1];
  if (e - b != 1 || (multi_wave & 4u)) {  // aggregates, or P = apk: the shared body
    set_pk_body(i, pk_off, pk_aff, pk_code, rand, P, set_code, n_bad, key_idx, tab_n, multi_wave, P2, comb);
    return;
  }
  // one key: set_pk_body / stage_set_pk's single-key branch, the table in LDS
  const uint64_t r = rand[i];
  if (P2) P2[i] = neg_r_g1(comb, r);
  g1a out;
  out.x = fp_zero();
  out.y = fp_zero();
  int code = TB_SUCCESS;
  uint32_t k;
  if (!set_key(key_idx, tab_n, b, k))
    code = TB_BAD_ENCODING;
  else if (pk_code[k] != TB_SUCCESS || r == 0)  // r == 0: [0] apk (a caller's randomizer is never 0)
    code = TB_PK_IS_INFINITY;
  else if (!jac_to_aff(out, mul_u64_aff_w2_lds(pk_aff[k], r, &tab[threadIdx.x])))
    code = TB_PK_IS_INFINITY;
  P[i] = out;
  if (code != TB_SUCCESS) {
    set_code[i] = (uint8_t)code;
    atomicAdd(n_bad, 1u);
  }
}

// k_set_pk_w2 for a device that keeps comb rows (tb_pkcomb.h):
// a single-key set whose key has a complete row takes [r] pk from it -- 15
// doublings and at most 16 mixed additions, no table to build -- and every
// other lane runs exactly what k_set_pk_w2 runs.  Which row: by index
// (key_idx) the table region's row key_idx itself, when the device has that
// region (tab_comb) -- every table key whose code is TB_SUCCESS has a row --
// else the key's reference word pk_ref[k] from k_pk_lookup_ref (the table
// region's row or the learned cache's, cache_comb; TB_PKREF_READY only when
// that row was complete before this batch began).  The same codes and n_bad as
// stage_set_pk.  comb_stat[0] += the sets multiplied through a row, one atomic
// per wave.
extern "C" __global__ void __launch_bounds__(TB_BLOCK, 2)
    k_set_pk_comb_w2(const uint32_t* __restrict__ pk_off, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code,
                     const uint64_t* __restrict__ rand, uint32_t n, g1a* __restrict__ P, uint8_t* __restrict__ set_code,
                     uint32_t* __restrict__ n_bad, const uint32_t* __restrict__ key_idx, uint32_t tab_n, uint32_t multi_wave,
                     g1a* __restrict__ P2, const g1a* __restrict__ comb, const uint32_t* __restrict__ pk_ref,
                     const g1a* __restrict__ cache_comb, const g1a* __restrict__ tab_comb, unsigned long long* __restrict__ comb_stat) {
  __shared__ g1a tab[3 * TB_BLOCK];  // the window path's table, as k_set_pk_w2's
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = pk_off[i], e = pk_off[i + 1];
  if (e - b != 1 || (multi_wave & 4u)) {
    set_pk_body(i, pk_off, pk_aff, pk_code, rand, P, set_code, n_bad, key_idx, tab_n, multi_wave, P2, comb);
    return;
  }
  const uint64_t r = rand[i];
  if (P2) P2[i] = neg_r_g1(comb, r);
  g1a out;
  out.x = fp_zero();
  out.y = fp_zero();
  int code = TB_SUCCESS;
  uint32_t k;
  const g1a* row = nullptr;
  if (!set_key(key_idx, tab_n, b, k))
    code = TB_BAD_ENCODING;
  else if (pk_code[k] != TB_SUCCESS || r == 0)
    code = TB_PK_IS_INFINITY;
  else if (key_idx) {
    if (tab_comb) row = tab_comb + (size_t)k * TB_PKCOMB_ENTRIES;
  } else if (pk_ref) {
    const uint32_t ref = pk_ref[k];
    if (ref & TB_PKREF_READY) row = ((ref & TB_PKREF_TABLE) ? tab_comb : cache_comb) + (size_t)(ref & TB_PKREF_ROW) * TB_PKCOMB_ENTRIES;
  }
  const unsigned long long served = __ballot(row != nullptr);  // the lanes here: the single-key sets of the wave
  if (row && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)served) - 1u) atomicAdd(comb_stat, (unsigned long long)__popcll(served));
  if (code == TB_SUCCESS) {
    const g1j rp = row ? comb_mul_u64(row, r) : mul_u64_aff_w2_lds(pk_aff[k], r, &tab[threadIdx.x]);
    if (!jac_to_aff(out, rp)) code = TB_PK_IS_INFINITY;
  }
  P[i] = out;
  if (code != TB_SUCCESS) {
    set_code[i] = (uint8_t)code;
    atomicAdd(n_bad, 1u);
  }
}
