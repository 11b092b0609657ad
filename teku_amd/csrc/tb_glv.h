// G1 scalar multiplication by an Fr scalar through the GLV endomorphism (the
// KZG kernels of k_kzg.hip; host-callable for the primitive tests of
// tests/native/tb_testops.h).
#pragma once
#include "tb_curve.h"
#include "tb_fr.h"

namespace tb {

// GLV split of a scalar k < r (plain limbs): k = a + b mu with a, b < 2^128,
// mu = z^2 the eigenvalue of phi(-P) = (beta x, -y) on G1.
// b = floor(k GLV_M / 2^384) (GLV_M = floor(2^384 / mu)) underestimates
// floor(k / mu) by at most 1 (the error is below k / 2^384 < 1; it is 1 for
// every multiple of mu); a = k - b mu is then corrected into [0, mu).
TB_HD TB_INLINE void glv_split(const fr& k, uint32_t (&a)[4], uint32_t (&b)[4]) {
  uint32_t prod[17];
  TB_UNROLL for (int i = 0; i < 17; i++) prod[i] = 0;
  TB_UNROLL for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
    TB_UNROLL for (int j = 0; j < 9; j++) {
      c = (uint64_t)k.l[i] * GLV_M[j] + prod[i + j] + (c >> 32);
      prod[i + j] = (uint32_t)c;
    }
    prod[i + 9] = (uint32_t)(c >> 32);
  }
  uint32_t q[5];
  TB_UNROLL for (int i = 0; i < 5; i++) q[i] = prod[12 + i];
  // rem = k - q mu (8 limbs; q mu <= k)
  uint32_t qm[9];
  TB_UNROLL for (int i = 0; i < 9; i++) qm[i] = 0;
  TB_UNROLL for (int i = 0; i < 5; i++) {
    uint64_t c = 0;
    TB_UNROLL for (int j = 0; j < 4; j++) {
      if (i + j < 9) {
        c = (uint64_t)q[i] * GLV_MU[j] + qm[i + j] + (c >> 32);
        qm[i + j] = (uint32_t)c;
      }
    }
    if (i + 4 < 9) qm[i + 4] = (uint32_t)(c >> 32);
  }
  uint32_t rem[8], br = 0;
  TB_UNROLL for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)k.l[i] - qm[i] - br;
    rem[i] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
  TB_UNROLL for (int it = 0; it < 2; it++) {  // rem >= mu ? rem -= mu, q += 1 (the second pass never subtracts)
    uint32_t t[8], bw = 0;
    TB_UNROLL for (int i = 0; i < 8; i++) {
      const uint64_t d = (uint64_t)rem[i] - (i < 4 ? GLV_MU[i] : 0u) - bw;
      t[i] = (uint32_t)d;
      bw = (uint32_t)(d >> 63);
    }
    const bool ge = bw == 0;
    uint32_t cq = ge ? 1u : 0u;
    TB_UNROLL for (int i = 0; i < 8; i++) rem[i] = ge ? t[i] : rem[i];
    TB_UNROLL for (int i = 0; i < 5; i++) {
      const uint64_t s = (uint64_t)q[i] + cq;
      q[i] = (uint32_t)s;
      cq = (uint32_t)(s >> 32);
    }
  }
  TB_UNROLL for (int i = 0; i < 4; i++) {
    a[i] = rem[i];
    b[i] = q[i];
  }
}

// [k]P, k in Montgomery form, P affine finite: [a]P + [b]phi(-P) by a joint
// MSB-first double-and-add over 128 bits (addends P, phi(-P), P + phi(-P),
// all affine) -- 128 doublings instead of 255.
TB_HD TB_INLINE g1j g1_mul_fr(const g1a& P, const fr& k_mont) {
  uint32_t a[4], b[4];
  glv_split(fr_from_mont(k_mont), a, b);
  g1a Q;
  Q.x = fp_mul(P.x, fp_from_const(BETA));
  Q.y = fp_neg(P.y);
  g1a S;
  (void)jac_to_aff(S, jac_add_aff(jac_from_aff(P), Q));  // P + [mu]P: never infinity (1 + mu != 0 mod r)
  g1j acc = jac_inf<fp>();
  TB_NOUNROLL for (int i = 127; i >= 0; --i) {
    acc = jac_dbl_i(acc);
    const bool ba = (a[i >> 5] >> (i & 31)) & 1u, bb = (b[i >> 5] >> (i & 31)) & 1u;
    if (ba || bb) {
      const g1a T = ba ? (bb ? S : P) : Q;
      acc = jac_add_aff_i(acc, T);
    }
  }
  return acc;
}

}  // namespace tb
