// The row point arithmetic (teku_amd/csrc/tb_cpoint.h) test ops, one definition
// for the host emulation (hostsim.cpp) and the GPU kernels (k_test_coop.hip),
// over G1 (J = cj1, F = c32) and G2 (J = cj2, F = c2).  Tests only.
//
// Inputs: affine P1 = (x1, y1), P2 = (x2, y2), the scalar k.  D = dbl(P1).
//   0: D                    1: madd(D, P2)           2: add(D, dbl(P2))
//   3: [k] P1 (mul_u64_aff) 4: [k] D (mul_u64)       5: [k]([k] P1)
// Exceptional cases (the caller passes P2 = 2 P1, so D and P2 are the same
// point in two representations); O = add(D, -P2) is the infinite point the
// formulas themselves produce:
//   8: madd(D, P2)          9: madd(D, -P2)
//  10: add(D, P2)          11: add(D, -P2)  (= O)
//  12: add(O, D)           13: add(D, O)            14: dbl(O)
// The header's promise is Z == 0 (mod p) for every one of 8..14.
#pragma once
#include "../../teku_amd/csrc/tb_cpoint.h"

namespace tb {
namespace coop {

TBC_FN c32 tneg(const c32& a) { return -a; }
TBC_FN c2 tneg(const c2& a) { return neg(a); }

template <typename J, typename F>
TBC_FN J cpoint_op(int op, const F& x1, const F& y1, const F& x2, const F& y2, const F& one, uint64_t k, const cctx& K) {
  const J p1 = {x1, y1, one};
  J r;
  if (op == 3 || op == 5)
    r = mul_u64_aff(x1, y1, k, one, K);
  else
    r = dbl(p1, K);
  if (op == 4 || op == 5) return mul_u64(r, k, K);
  if (op == 0 || op == 3) return r;
  if (op == 1 || op == 8 || op == 9) return madd(r, x2, op == 9 ? tneg(y2) : y2, K);
  J s = {x2, op >= 11 ? tneg(y2) : y2, one};
  if (op == 2) s = dbl(s, K);
  // one add instance: the second pass (12, 13) feeds O back as an operand
  J a = r, b = s, t = r;
  const int passes = (op == 12 || op == 13) ? 2 : 1;
  TB_NOUNROLL for (int i = 0; i < passes; i++) {
    t = add(a, b, K);
    a = op == 12 ? t : r;
    b = op == 12 ? r : t;
  }
  if (op == 14) t = dbl(t, K);
  return t;
}

}  // namespace coop
}  // namespace tb
