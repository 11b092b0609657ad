// Fixed-base comb tables for keys the device keeps: [r] pk for
// a 64-bit r in 15 doublings and at most 16 mixed additions, from 15 affine
// multiples of pk computed once per key.
//
//  * four teeth 16 bits apart: entry d (1..15) is T[d] = sum over the set bits
//    t of d of 2^(16 t) pk, affine, at g1a index d - 1 of the key's row
//    (TB_PKCOMB_ROW_BYTES = 15 x 96 bytes, the word order of a cache row's
//    point);
//  * column j (15..0) of r has the digit whose bit t is r's bit 16 t + j; the
//    walk starts at the highest column with a non-zero digit, doubles once per
//    column below it and adds the column's entry when its digit is not zero;
//  * no addition is exceptional: before the addition at column j the running
//    scalar has bits only at positions 16 t + s with 1 <= s <= 15 (every
//    earlier column was doubled at least once since it was added), the entry
//    only at positions 16 t; the two differ, neither is zero, and both are
//    below 2^64, far below the group order, so the running point is never
//    plus or minus the addend (jac_add_aff_i's branch is never taken).  The
//    same holds inside comb_build: its sums are of distinct multiples of pk
//    below 2^49.
//
// Host and device run the same functions: the product builds and reads the
// rows on the device only (k_pkindex.hip k_pk_learn_comb and k_pk_comb_build,
// k_w2_pk.hip k_set_pk_comb_w2); tests/native/pkcomb_check.cpp runs them on
// the CPU.
#pragma once
#include "tb_curve.h"

#define TB_PKCOMB_ENTRIES 15u
#define TB_PKCOMB_ROW_BYTES (TB_PKCOMB_ENTRIES * 96u)

// A batch key's reference (k_pk_lookup_ref writes one word per key, the comb
// kernel reads it): where the lookup found the key, and whether that row's
// comb may be read.  0: not found, or no comb row.
#define TB_PKREF_NONE 0u
#define TB_PKREF_READY 0x80000000u  // the row's 15 entries are complete
#define TB_PKREF_TABLE 0x40000000u  // a row of the loaded table's region, else of the learned cache's
#define TB_PKREF_ROW 0x3fffffffu

namespace tb {

static_assert(sizeof(g1a) == 96, "a comb entry is a 96-byte affine point");

// A cache row's comb may be written and read: the row lies below the comb
// region's cap (TBLS_PK_COMB_KEYS).  Rows at or beyond it never become ready.
TB_HD TB_INLINE bool comb_row_in_cap(uint32_t row, uint32_t cap) { return row < cap; }
TB_HD TB_INLINE uint32_t comb_ref(bool table, uint32_t row, bool ready) {
  return ready ? (TB_PKREF_READY | (table ? TB_PKREF_TABLE : 0u) | (row & TB_PKREF_ROW)) : TB_PKREF_NONE;
}
// After comb_build of a published cache row: set its ready byte (row < cap).
TB_HD TB_INLINE void comb_mark_ready(uint8_t* ready, uint32_t row, uint32_t cap) {
  if (comb_row_in_cap(row, cap)) ready[row] = 1;
}

// The digit of column j (0..15) of r.
TB_HD TB_INLINE uint32_t comb_digit(uint64_t r, int j) {
  const uint64_t s = r >> j;
  return (uint32_t)(s & 1u) | (uint32_t)((s >> 15) & 2u) | (uint32_t)((s >> 30) & 4u) | (uint32_t)((s >> 45) & 8u);
}

// comb_build's working memory: TB_PKCOMB_TMP field elements at tmp[k * stride]
// (the device gives each lane a column of LDS, the host an array).
#define TB_PKCOMB_TMP 14u

// Jacobian results parked in the row: X, Y in entry d's place, Z in tmp[k].
TB_HD TB_INLINE void comb_park(g1a* row, fp* tmp, uint32_t stride, uint32_t d, uint32_t k, const g1j& J) {
  row[d - 1] = g1a{J.x, J.y};
  tmp[k * stride] = J.z;
}
TB_HD TB_INLINE g1j comb_parked(const g1a* row, const fp* tmp, uint32_t stride, uint32_t d, uint32_t k) {
  return g1j{row[d - 1].x, row[d - 1].y, tmp[k * stride]};
}
// The seven parked results of entries lo .. lo + 6 (Z in tmp[0 .. 7)) to affine
// with one inversion (Montgomery's trick; the prefix products in tmp[7 .. 14)).
TB_HD inline void comb_normalize7(g1a* row, fp* tmp, uint32_t stride, uint32_t lo) {
  tmp[7 * stride] = tmp[0];
  TB_NOUNROLL for (uint32_t k = 1; k < 7; k++) tmp[(7 + k) * stride] = fp_mul(tmp[(6 + k) * stride], tmp[k * stride]);
  fp inv = fp_inv(tmp[13 * stride]);
  TB_NOUNROLL for (uint32_t k = 7; k-- > 0;) {
    fp zi = inv;
    if (k) {
      zi = fp_mul(inv, tmp[(6 + k) * stride]);
      inv = fp_mul(inv, tmp[k * stride]);
    }
    const fp zi2 = fp_sqr(zi);
    const g1a e = row[lo - 1 + k];
    row[lo - 1 + k] = g1a{fp_mul(e.x, zi2), fp_mul(fp_mul(e.y, zi2), zi)};
  }
}

// The 15 entries of the finite affine key P into row[0 .. 15).  Entries 2..8
// first: 48 doublings for 2^16 P, 2^32 P and 2^48 P and four additions, brought
// to affine with one shared inversion; then entries 9..15 = T[8] + T[d], mixed
// additions of affine points, with a second one.  (One inversion over all 14
// would hold 28 field elements per lane; the two halves hold 14, which on the
// device is LDS instead of scratch, and the second half's additions are the
// cheaper mixed ones.)  The row itself is the only other storage.
TB_HD inline void comb_build(g1a* row, const g1a& P, fp* tmp, uint32_t stride) {
  row[0] = P;
  g1j t = jac_from_aff(P);
  TB_NOUNROLL for (uint32_t tooth = 1; tooth < 4; tooth++) {
    TB_NOUNROLL for (int i = 0; i < 16; i++) t = jac_dbl_i(t);
    comb_park(row, tmp, stride, 1u << tooth, (1u << tooth) - 2u, t);  // d = 2, 4, 8 at k = d - 2
  }
  comb_park(row, tmp, stride, 3, 1, jac_add_aff(comb_parked(row, tmp, stride, 2, 0), P));
  comb_park(row, tmp, stride, 5, 3, jac_add_aff(comb_parked(row, tmp, stride, 4, 2), P));
  comb_park(row, tmp, stride, 6, 4, jac_add(comb_parked(row, tmp, stride, 4, 2), comb_parked(row, tmp, stride, 2, 0)));
  comb_park(row, tmp, stride, 7, 5, jac_add(comb_parked(row, tmp, stride, 4, 2), comb_parked(row, tmp, stride, 3, 1)));
  comb_normalize7(row, tmp, stride, 2);
  const g1j T8 = jac_from_aff(row[7]);
  TB_NOUNROLL for (uint32_t d = 1; d < 8; d++) comb_park(row, tmp, stride, 8 + d, d - 1, jac_add_aff(T8, row[d - 1]));
  comb_normalize7(row, tmp, stride, 9);
}

// [r] pk from pk's row, r != 0, Jacobian.  Each step reads its column's entry
// first (a zero digit reads entry 0 and adds nothing, so the read is
// unconditional), then doubles, then adds: the entry is not needed until the
// doubling is done, which leaves the compiler free to keep the 96-byte gather
// in flight under it.  Whether it does has not been checked in the ISA.
TB_HD TB_INLINE g1j comb_mul_u64(const g1a* row, uint64_t r) {
  int j = 15;
  uint32_t d = comb_digit(r, j);
  while (d == 0) d = comb_digit(r, --j);  // r != 0: some column has a digit
  g1j acc = jac_from_aff(row[d - 1]);
  TB_NOUNROLL for (--j; j >= 0; --j) {
    d = comb_digit(r, j);
    const g1a e = row[d ? d - 1 : 0];
    acc = jac_dbl_i(acc);
    if (d) acc = jac_add_aff_i(acc, e);
  }
  return acc;
}

}  // namespace tb
