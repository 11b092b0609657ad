// Small-batch key and signature stages, lane-cooperative (tb_ccurve.h): the
// p50 path's per-set chains at <= TB_HASH_WAVE_MAX sets, where one thread per
// set (k_pk_decompress -> k_set_pk, k_sig_check) leaves the chip idle and the
// latency of lone-lane products sets the time.
//
//   k_keys_coop       4 sets per 128-thread workgroup (row r of each wave = set
//                     4 b + r).  Wave 0: key decode, the square root, the G1
//                     subgroup check; wave 1: -[r] g1 from the comb, then
//                     [r] pk, one shared inversion, both points affine.  Same
//                     outputs as k_pk_decompress + k_set_pk (P, P2, set_code,
//                     n_bad) for sets of one key; other sets (never selected by
//                     the host, kept correct) run the one-lane stage bodies.
//   k_sig_check_coop  4 sets per 64-thread wave: decode, Fp2 square root (two
//                     coop exponentiations), G2 subgroup check; the outputs of
//                     k_sig_check in skip mode 1.
// Further down: the multi-key aggregation (k_set_pk_agg_coop), the
// sync-committee bit rows (k_set_pk_bits_coop) and the per-group sums of
// grouped batches (k_group_items, k_group_pk_sum_coop) on the same 32-row layout.
#include "tb_kdecl.h"
#include "tb_comb.h"
#include "tb_ccurve.h"

using namespace tb;
using coop::c32;

#define KC_PENDING (-1)

struct kc_set {
  int32_t zb0[4][16], zb1[4][16];
  fp x, y, inv;
  fp out[4];
  int code;
  uint32_t want;
};

// lane 0 of a row: the 48-byte key up to the square root (g1_decompress);
// KC_PENDING with x (Montgomery) or the set's failure code (any invalid key:
// PK_IS_INFINITY, stage_set_pk)
__device__ TB_INLINE int kc_decode(const uint8_t* b, fp& x, uint32_t& want) {
  const uint8_t b0 = b[0];
  want = (b0 & 0x20) ? 1u : 0u;
  if (!(b0 & 0x80) || (b0 & 0x40)) return TB_PK_IS_INFINITY;  // bad encoding or the infinity key
  fp v = fp_plain_from_be(b);
  v.l[11] &= 0x1fffffffu;
  if (!fp_plain_lt_p(v) || fp_is_zero(v)) return TB_PK_IS_INFINITY;  // x = 0: (0, +-2) has order 3
  x = fp_to_mont(v);
  return KC_PENDING;
}

// a set of other than one key: the one-lane bodies (decode + check each key)
__device__ TB_NOINLINE int kc_set_generic(const uint8_t* pks, const g1a* tab_aff, const uint8_t* tab_code, const uint32_t* key_idx,
                                          uint32_t tab_n, uint32_t b, uint32_t e, uint64_t r, g1a& o) {
  if (!pks) return stage_set_pk(tab_aff, tab_code, b, e, r, o, key_idx, tab_n);
  o.x = fp_zero();
  o.y = fp_zero();
  g1j acc = jac_inf<fp>();
  for (uint32_t j = b; j < e; j++) {
    g1a a;
    if (stage_pk(pks + (size_t)j * 48, a) != TB_SUCCESS) return TB_PK_IS_INFINITY;
    acc = jac_add_aff(acc, a);
  }
  return stage_set_pk_finish(acc, r, o);
}

// -[r] g1 of a set whose row held no valid single key, on one lane (neg_r_g1)
__device__ TB_NOINLINE g1a kc_neg_r_g1(const g1a* comb, uint64_t r) { return neg_r_g1(comb, r); }

// pks: 48-byte keys, or nullptr with (tab_aff, tab_code, key_idx, tab_n): keys
// from the device-resident table.  P2 nullable.
extern "C" __global__ void __launch_bounds__(128)
    k_keys_coop(const uint8_t* __restrict__ pks, const uint32_t* __restrict__ pk_off, const g1a* __restrict__ tab_aff,
                const uint8_t* __restrict__ tab_code, const uint32_t* __restrict__ key_idx, uint32_t tab_n,
                const uint64_t* __restrict__ rand, uint32_t n, g1a* __restrict__ P, g1a* __restrict__ P2,
                uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad, const g1a* __restrict__ comb) {
  __shared__ kc_set S[4];
  tb_latency_prio();
  const int w = threadIdx.x >> 6, r = (threadIdx.x >> 4) & 3, d = crow::dig();
  const uint32_t i = blockIdx.x * 4 + r;
  const bool act = i < n;
  kc_set& M = S[r];
  const coop::cctx K = coop::cctx_load();
  uint32_t b = 0, e = 0;
  uint64_t rnd = 0;
  if (act) {
    b = pk_off[i];
    e = pk_off[i + 1];
    rnd = rand[i];
  }
  const bool single = act && e - b == 1;
  const c32 one = crow::from_const(R1);
  coop::cj1 cacc = {c32(0), c32(0), one};
  bool cinf = true;
  if (w == 0) {
    // ---- the key: decode + square root (rows compute in step; rows without a
    // pending key run on zeros and keep their code)
    if (d == 0) {
      fp x = fp_zero(), y = fp_zero();
      uint32_t want = 0;
      int code = TB_PK_IS_INFINITY;
      if (single) {
        if (pks) {
          code = kc_decode(pks + (size_t)b * 48, x, want);
        } else {
          uint32_t k;
          if (!set_key(key_idx, tab_n, b, k))
            code = TB_BAD_ENCODING;
          else if (tab_code[k] != TB_SUCCESS)
            code = TB_PK_IS_INFINITY;
          else {
            x = tab_aff[k].x;
            y = tab_aff[k].y;
            code = TB_SUCCESS;
          }
        }
      }
      M.x = x;
      M.y = y;
      M.want = want;
      M.code = code;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (pks) {
      const c32 x = crow::from_fp(M.x);
      const c32 rhs = coop::cnorm(coop::cmul(coop::csqr(x, K), x, K) + crow::from_const(B_G1));
      c32 a1[1] = {rhs}, y1[1];
      coop::cpow_win_n<1>(y1, a1, EXPW_SQRT_FIRST, EXPW_SQRT, EXPW_SQRT_N, K);
      const c32 v[2] = {coop::csqr(y1[0], K) - rhs, y1[0]};
      crow::to_fp_n<2>(v, M.zb0, M.out);
      if (d == 0 && M.code == KC_PENDING) {
        if (!fp_is_zero(M.out[0])) {
          M.code = TB_PK_IS_INFINITY;  // not on the curve
        } else {
          const fp y = M.out[1];
          M.y = fp_cneg(y, fp_sign_zcash(y) != (M.want != 0));
        }
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  } else {
    // ---- -[r] g1: one mixed addition per nonzero byte of r (neg_r_g1)
    for (int k = 0; k < 8; k++) {
      const uint32_t dg = (uint32_t)(rnd >> (8 * k)) & 255u;
      if (dg) {
        const g1a* q = comb + k * 256 + dg;
        const c32 qx = crow::from_fp(q->x), qy = crow::from_fp(q->y);
        if (cinf) {
          cacc = {qx, qy, one};
          cinf = false;
        } else {
          cacc = coop::madd(cacc, qx, qy, K);
        }
      }
    }
  }
  __syncthreads();
  if (w == 0) {
    if (pks) {  // ---- G1 subgroup check
      const bool ok = crow::g1_in_group(crow::from_fp(M.x), crow::from_fp(M.y), M.zb0, K);
      if (d == 0 && M.code == KC_PENDING) M.code = ok ? TB_SUCCESS : TB_PK_IS_INFINITY;
    }
  } else {
    // ---- [r] pk (invalid keys: garbage, their code decides), one inversion
    // for Z of [r] pk and of the comb sum, both points affine
    const c32 x = crow::from_fp(M.x), y = crow::from_fp(M.y);
    const coop::cj1 t = coop::mul_u64_aff(x, y, rnd ? rnd : 1ull, one, K);
    const c32 zc = cacc.z;
    const c32 v1[1] = {coop::cmul(t.z, zc, K)};
    crow::to_fp_n<1>(v1, M.zb1, &M.inv);
    {
      const fp z = cinv::inv_row_lane0(M.inv, M.zb1[0]);  // the row's inversion (tb_cinv.h)
      if (d == 0) M.inv = z;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const c32 iv = crow::from_fp(M.inv);
    c32 a1[2] = {iv, iv}, b1[2] = {zc, t.z}, i1[2];
    coop::cmul_n<2>(i1, a1, b1, K);  // 1 / Z_t, 1 / Z_c
    c32 i2[2];
    coop::cmul_n<2>(i2, i1, i1, K);
    c32 a3[4] = {t.x, cacc.x, i2[0], i2[1]}, b3[4] = {i2[0], i2[1], i1[0], i1[1]}, i3[4];
    coop::cmul_n<4>(i3, a3, b3, K);
    c32 a4[2] = {t.y, cacc.y}, b4[2] = {i3[2], i3[3]}, i4[2];
    coop::cmul_n<2>(i4, a4, b4, K);
    const c32 v4[4] = {i3[0], i4[0], i3[1], i4[1]};
    crow::to_fp_n<4>(v4, M.zb1, M.out);
  }
  __syncthreads();
  if (w == 1 && d == 0 && act) {
    if (P2) {
      g1a o;
      if (!single || M.code != TB_SUCCESS) {
        // the row multiplied zeros or an invalid key: Z = 0 there zeroes the
        // inversion both points share, so this set's -[r] g1 comes from one lane
        o = kc_neg_r_g1(comb, rnd);
      } else if (cinf) {
        o.x = fp_zero();
        o.y = fp_neg(fp_zero());
      } else {
        o.x = M.out[2];
        o.y = fp_neg(M.out[3]);
      }
      P2[i] = o;
    }
    g1a o;
    o.x = fp_zero();
    o.y = fp_zero();
    int code;
    if (!single) {
      code = kc_set_generic(pks, tab_aff, tab_code, key_idx, tab_n, b, e, rnd, o);
    } else {
      code = M.code;
      if (code == TB_SUCCESS && rnd == 0) code = TB_PK_IS_INFINITY;  // [0] pk: infinity
      if (code == TB_SUCCESS) {
        o.x = M.out[0];
        o.y = M.out[1];
      }
    }
    P[i] = o;
    if (code != TB_SUCCESS) {
      set_code[i] = (uint8_t)code;
      atomicAdd(n_bad, 1u);
    }
  }
}

// ---------------------------------------------------------------------------
struct ks_set {
  int32_t zb[6][16];
  fp2 x, y;
  fp out[4];
  int code;
  uint32_t want, inf, xzero;
};

// k_sig_check, skip mode 1: sig_aff = Q of the set's signature pair, sig_use =
// its skip flag (1: no pair -- infinite or invalid)
extern "C" __global__ void __launch_bounds__(64)
    k_sig_check_coop(const uint8_t* __restrict__ sigs, uint32_t n, g2a* __restrict__ sig_aff, uint8_t* __restrict__ sig_use,
                     uint8_t* __restrict__ sig_code, uint32_t* __restrict__ n_bad) {
  __shared__ ks_set S[4];
  tb_latency_prio();
  const int r = (threadIdx.x >> 4) & 3, d = crow::dig();
  const uint32_t i = blockIdx.x * 4 + r;
  const bool act = i < n;
  ks_set& M = S[r];
  const coop::cctx K = coop::cctx_load();
  if (d == 0) {  // g2_decompress up to the square root
    fp2 x = fp2_zero();
    int code = TB_BAD_ENCODING;
    uint32_t inf = 0, want = 0;
    if (act) {
      const uint8_t* bb = sigs + (size_t)i * 96;
      const uint8_t b0 = bb[0];
      want = (b0 & 0x20) ? 1u : 0u;
      if (!(b0 & 0x80)) {
        code = TB_BAD_ENCODING;
      } else if (b0 & 0x40) {
        uint32_t acc = b0 & 0x3f;
        for (int k = 1; k < 96; k++) acc |= bb[k];
        code = acc ? TB_BAD_ENCODING : TB_SUCCESS;
        inf = acc ? 0u : 1u;
      } else {
        fp x1 = fp_plain_from_be(bb);
        x1.l[11] &= 0x1fffffffu;
        const fp x0 = fp_plain_from_be(bb + 48);
        if (!fp_plain_lt_p(x1) || !fp_plain_lt_p(x0)) {
          code = TB_BAD_ENCODING;
        } else {
          x = {fp_to_mont(x0), fp_to_mont(x1)};
          code = KC_PENDING;
        }
      }
    }
    M.x = x;
    M.code = code;
    M.inf = inf;
    M.want = want;
    M.xzero = fp2_is_zero(x) ? 1u : 0u;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  // ---- y = sqrt(x^3 + 4(1 + u)) (fp2_sqrt: gamma = sqrt N, delta, s)
  const crow::c2 x = crow::from_fp2(M.x);
  const crow::c2 a = crow::norm(crow::add(crow::mul(crow::sqr(x, K), x, K), crow::from_const2(B_G2)));
  c32 g1[1];
  {
    c32 n1[1] = {coop::cnorm(crow::norm2(a, K))};
    coop::cpow_win_n<1>(g1, n1, EXPW_SQRT_FIRST, EXPW_SQRT, EXPW_SQRT_N, K);
  }
  const c32 half = crow::from_const(FP_HALF);
  c32 dl[2];
  {
    c32 p[2] = {coop::cnorm(a.c0 + g1[0]), coop::cnorm(a.c0 - g1[0])}, h[2] = {half, half};
    coop::cmul_n<2>(dl, p, h, K);
  }
  const c32 z1[1] = {dl[0]};
  const c32 delta = crow::zeros_n<1>(z1, M.zb) ? dl[1] : dl[0];
  c32 s1[1];
  {
    c32 d1[1] = {delta};
    coop::cpow_win_n<1>(s1, d1, EXPW_PM3D4_FIRST, EXPW_PM3D4, EXPW_PM3D4_N, K);
  }
  const c32 s = s1[0];
  c32 t1[2];
  {
    c32 p[2] = {s, a.c1}, q[2] = {delta, s};
    coop::cmul_n<2>(t1, p, q, K);  // s delta, a1 s
  }
  c32 t2[2];
  {
    c32 p[2] = {s, t1[1]}, q[2] = {t1[0], half};
    coop::cmul_n<2>(t2, p, q, K);  // chi = s^2 delta, a1 s / 2
  }
  const c32 zc[1] = {t2[0] - crow::from_const(R1)};
  const bool pos = crow::zeros_n<1>(zc, M.zb) != 0;
  const crow::c2 y = pos ? crow::c2{t1[0], t2[1]} : crow::c2{-t2[1], t1[0]};
  const crow::c2 yy = crow::sqr(y, K);
  const c32 v[4] = {yy.c0 - a.c0, yy.c1 - a.c1, y.c0, y.c1};
  crow::to_fp_n<4>(v, M.zb, M.out);
  if (d == 0 && M.code == KC_PENDING) {
    if (!fp_is_zero(M.out[0]) || !fp_is_zero(M.out[1])) {
      M.code = TB_POINT_NOT_ON_CURVE;
    } else {
      fp2 yf = {M.out[2], M.out[3]};
      if (fp2_sign_zcash(yf) != (M.want != 0)) yf = fp2_neg(yf);
      M.y = yf;
      if (M.xzero) M.code = TB_POINT_NOT_IN_GROUP;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  // ---- G2 subgroup check (rows without a pending point run on their values)
  const bool ok = crow::g2_in_group(x, crow::from_fp2(M.y), M.zb, K);
  if (d == 0 && act) {
    int code = M.code;
    if (code == KC_PENDING) code = ok ? TB_SUCCESS : TB_POINT_NOT_IN_GROUP;
    const bool use = code == TB_SUCCESS && !M.inf;
    g2a o;
    o.x = use ? M.x : fp2_zero();
    o.y = use ? M.y : fp2_zero();
    sig_aff[i] = o;
    sig_use[i] = use ? 0 : 1;
    sig_code[i] = (uint8_t)code;
    if (code != TB_SUCCESS) atomicAdd(n_bad, 1u);
  }
}

// ---------------------------------------------------------------------------
// Multi-key sets (configs 2/3: 488-512 keys per set; BlstPublicKey.aggregate,
// BlstPublicKey.java:55-71), lane-cooperative: one 512-thread workgroup (32
// rows, 256 registers each) per set of the compacted list.
//   * row q sums the set's keys q, q + 32, ... with coop mixed additions, and
//     the 32 row sums meet in a 5-level LDS tree of coop additions;
//   * P = [r] apk by nibbles: row w < 16 forms [r_w] (2^(4w) apk) (4w
//     doublings, then a 4-bit double-and-add), the 16 terms meet in a 4-level
//     tree -- the critical path is the 63 doublings of row 15 plus 7 additions
//     instead of 63 doublings and ~32 additions in one chain;
//   * row 16 (wave 4, beside it): the set's signature-pair point -[r] g1 from
//     the comb (P2, when given); both points affine with one lane-0
//     inversion each.
// The coop additions have no exceptional-case branches: a sum that meets
// P == +-Q (a repeated key, or keys cancelling) ends with Z = 0 and stays
// there through every later addition, so Z = 0 of the aggregate sends the set
// to lane 0's one-lane body (stage_set_pk: exact, and infinity ->
// PK_IS_INFINITY).  For a finite aggregate of group points the nibble terms
// [k 2^(4w)] apk (1 <= k <= 15) and their partial sums over disjoint nibbles
// never meet +-each other (distinct multiples below 2^64 < r), so [r] apk is
// exact.  Same outputs as k_set_pk_wave.
// ---------------------------------------------------------------------------
#define KA_ROWS 32
struct ka_set {
  int32_t pt[KA_ROWS][3][16];  // row sums (X, Y, Z digits), then the nibble terms
  uint32_t inf[KA_ROWS];
  int32_t zb[2][4][16];        // row 0 ([r] apk) and row 16 (-[r] g1)
  fp inv[2];
  fp out[2][2];
  int bad;
  int mode;  // 0: nibble [r] apk, 1: one-lane fallback, 2: the set fails (code in bad)
};

__device__ TB_NOINLINE int ka_set_generic(const g1a* pk_aff, const uint8_t* pk_code, uint32_t b, uint32_t e, uint64_t r, g1a& o,
                                          const uint32_t* key_idx, uint32_t tab_n) {
  return stage_set_pk(pk_aff, pk_code, b, e, r, o, key_idx, tab_n);
}

// rows q < rows hold points (pt, inf); tree them into row 0 (all threads call)
__device__ TB_INLINE void ka_tree(ka_set& S, int rows, int q, int d, const coop::cctx& K) {
  for (int s = rows / 2; s > 0; s >>= 1) {
    coop::cj1 acc = {c32(0), c32(0), c32(0)};
    if (q < s && S.inf[q + s] == 0) {
      const coop::cj1 o = {S.pt[q + s][0][d], S.pt[q + s][1][d], S.pt[q + s][2][d]};
      if (S.inf[q] == 0) {
        const coop::cj1 m = {S.pt[q][0][d], S.pt[q][1][d], S.pt[q][2][d]};
        acc = coop::add(m, o, K);
      } else {
        acc = o;
      }
    }
    __syncthreads();
    if (q < s && S.inf[q + s] == 0) {
      S.pt[q][0][d] = acc.x;
      S.pt[q][1][d] = acc.y;
      S.pt[q][2][d] = acc.z;
      if (d == 0) S.inf[q] = 0u;
    }
    __syncthreads();
  }
}

// (X, Y, Z) -> affine into out[0..1] with one lane-0 inversion (zb, inv: the row's buffers)
__device__ TB_INLINE void ka_affine(const coop::cj1& t, int32_t (*zb)[16], fp& inv, fp* out, int d, const coop::cctx& K) {
  const c32 v1[1] = {t.z};
  crow::to_fp_n<1>(v1, zb, &inv);
  {
    const fp z = cinv::inv_row_lane0(inv, zb[0]);  // the row's inversion (tb_cinv.h)
    if (d == 0) inv = z;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const c32 i1 = crow::from_fp(inv);
  const c32 i2 = coop::csqr(i1, K);
  c32 a3[2] = {t.x, i2}, b3[2] = {i2, i1}, i3[2];
  coop::cmul_n<2>(i3, a3, b3, K);  // X / Z^2, 1 / Z^3
  const c32 y = coop::cmul(t.y, i3[1], K);
  const c32 v2[2] = {i3[0], y};
  crow::to_fp_n<2>(v2, zb, out);
}

// The tail the multi-key kernels share (all threads call, after the row tree):
// row 0 of S.pt / S.inf holds the set's aggregate, S.bad an invalid key's
// code.  Z = 0 or infinity sends the set to gen(r, o), the caller's exact
// one-lane body; otherwise P[i] = [rnd] apk by nibbles, and P2[i] = -[r] g1
// (when P2 is given) on row 16; failures go to set_code / n_bad.
template <class GEN>
__device__ TB_INLINE void ka_finish(ka_set& S, uint32_t i, uint64_t rnd, const uint64_t* __restrict__ rand, g1a* __restrict__ P,
                                    g1a* __restrict__ P2, uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad,
                                    const g1a* __restrict__ comb, int q, int d, const coop::cctx& K, const c32& one, const GEN& gen) {
  // ---- the aggregate: exceptional / infinite -> one-lane body; invalid key or r = 0 -> fail
  if (q == 0) {
    const c32 zv[1] = {S.pt[0][2][d]};
    const bool zero = S.inf[0] != 0 || crow::zeros_n<1>(zv, S.zb[0]) != 0u;
    if (d == 0) {
      int mode = 0;
      if (S.bad != TB_SUCCESS) {
        mode = 2;
      } else if (zero) {
        mode = 1;
      } else if (rnd == 0) {
        S.bad = TB_PK_IS_INFINITY;  // [0] apk (stage_set_pk_finish)
        mode = 2;
      }
      S.mode = mode;
    }
  }
  __syncthreads();
  const int mode = S.mode;
  // ---- row 16: -[r] g1 (one mixed addition per nonzero byte of r: neg_r_g1)
  if (q == 16 && P2) {
    const uint64_t rr = rand[i];
    coop::cj1 cacc = {one, one, c32(0)};
    bool cinf = true;
    for (int k = 0; k < 8; k++) {
      const uint32_t dg = (uint32_t)(rr >> (8 * k)) & 255u;
      if (dg) {
        const g1a* cq = comb + k * 256 + dg;
        const c32 qx = crow::from_fp(cq->x), qy = crow::from_fp(cq->y);
        if (cinf) {
          cacc = {qx, qy, one};
          cinf = false;
        } else {
          cacc = coop::madd(cacc, qx, qy, K);
        }
      }
    }
    if (!cinf) ka_affine(cacc, S.zb[1], S.inv[1], S.out[1], d, K);
    if (d == 0) {
      g1a o;
      o.x = cinf ? fp_zero() : S.out[1][0];
      o.y = fp_neg(cinf ? fp_zero() : S.out[1][1]);
      P2[i] = o;
    }
  }
  // ---- [r] apk by nibbles on rows 0..15
  coop::cj1 t = {c32(0), c32(0), c32(0)};
  bool tinf = true;
  if (mode == 0 && q < 16) {
    const uint32_t nib = (uint32_t)(rnd >> (4 * q)) & 15u;
    if (nib) {
      coop::cj1 a = {S.pt[0][0][d], S.pt[0][1][d], S.pt[0][2][d]};
      for (int k = 0; k < 4 * q; k++) a = coop::dbl(a, K);  // 2^(4q) apk
      t = a;
      for (int bit = 31 - __builtin_clz(nib) - 1; bit >= 0; --bit) {
        t = coop::dbl(t, K);
        if ((nib >> bit) & 1u) t = coop::add(t, a, K);
      }
      tinf = false;
    }
  }
  __syncthreads();  // every row has read the aggregate
  if (mode == 0 && q < 16) {
    S.pt[q][0][d] = t.x;
    S.pt[q][1][d] = t.y;
    S.pt[q][2][d] = t.z;
    if (d == 0) S.inf[q] = tinf ? 1u : 0u;
  }
  __syncthreads();
  if (mode == 0) ka_tree(S, 16, q, d, K);
  if (q == 0) {
    int code = S.bad;
    if (mode == 0) {
      const coop::cj1 rp = {S.pt[0][0][d], S.pt[0][1][d], S.pt[0][2][d]};
      ka_affine(rp, S.zb[0], S.inv[0], S.out[0], d, K);
    } else if (mode == 1 && d == 0) {  // infinity or an exceptional addition: the exact one-lane body
      g1a o;
      code = gen(rnd, o);
      S.out[0][0] = o.x;
      S.out[0][1] = o.y;
    }
    if (d == 0) {  // lane 0's code is the set's in every mode
      g1a o;
      o.x = fp_zero();
      o.y = fp_zero();
      if (code == TB_SUCCESS) {
        o.x = S.out[0][0];
        o.y = S.out[0][1];
      } else {
        set_code[i] = (uint8_t)code;
        atomicAdd(n_bad, 1u);
      }
      P[i] = o;
    }
  }
}

extern "C" __global__ void __launch_bounds__(KA_ROWS * 16)
    k_set_pk_agg_coop(const uint32_t* __restrict__ pk_off, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code,
                      const uint64_t* __restrict__ rand, const uint32_t* __restrict__ list, const uint32_t* __restrict__ cnt,
                      g1a* __restrict__ P, uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad,
                      const uint32_t* __restrict__ key_idx, uint32_t tab_n, g1a* __restrict__ P2, const g1a* __restrict__ comb,
                      uint32_t unit_r) {
  __shared__ ka_set S;
  tb_latency_prio();
  const int q = crow::row(), d = crow::dig();
  const coop::cctx K = coop::cctx_load();
  const c32 one = crow::from_const(R1);
  const uint32_t total = cnt[0];
  for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint32_t i = list[w], b = pk_off[i], e = pk_off[i + 1];
    const uint64_t rnd = unit_r ? 1ull : rand[i];  // unit_r: r multiplies H(m) instead (k_set_hash_coop)
    if (threadIdx.x == 0) S.bad = TB_SUCCESS;
    __syncthreads();
    // ---- row sums (row-uniform control flow: every lane of a row walks the same keys)
    coop::cj1 acc = {c32(0), c32(0), c32(0)};
    bool inf = true;
    for (uint32_t j = b + (uint32_t)q; j < e; j += KA_ROWS) {
      uint32_t k;
      if (!set_key(key_idx, tab_n, j, k)) {
        S.bad = TB_BAD_ENCODING;
      } else if (pk_code[k] != TB_SUCCESS) {
        S.bad = TB_PK_IS_INFINITY;  // BlstPublicKey.java:58-65 (any racing writer stores a failure)
      } else {
        const c32 qx = crow::from_fp(pk_aff[k].x), qy = crow::from_fp(pk_aff[k].y);
        if (inf) {
          acc = {qx, qy, one};
          inf = false;
        } else {
          acc = coop::madd(acc, qx, qy, K);
        }
      }
    }
    S.pt[q][0][d] = acc.x;
    S.pt[q][1][d] = acc.y;
    S.pt[q][2][d] = acc.z;
    if (d == 0) S.inf[q] = inf ? 1u : 0u;
    __syncthreads();
    ka_tree(S, KA_ROWS, q, d, K);
    ka_finish(S, i, rnd, rand, P, P2, set_code, n_bad, comb, q, d, K, one, [&](uint64_t r, g1a& o) {
      return ka_set_generic(pk_aff, pk_code, b, e, r, o, key_idx, tab_n);
    });
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Sync-committee sets from a resident committee and a participation bitfield
// (BlockProcessorAltair.java:234-267: the committee's keys whose bit is set,
// in committee order, to BLS.fastAggregateVerify, BLS.java:185-207).  The
// committee is a list of table indices (members), its bad-member mask and the
// affine sum of its valid members (k_committee_mask + one set of this kernel
// at load time).  One 512-thread workgroup per set, the layout and outputs of
// k_set_pk_agg_coop:
//   * the set's bit row is staged in LDS (at most 256 B), its participants
//     (c) and absent valid members (a) counted, and ANDed with the bad-member
//     mask: a participating invalid member fails the set (PK_IS_INFINITY);
//   * a < c with a usable committee sum: the rows walk the ABSENT valid
//     members and add their negations, the row tree meets them and row 0 adds
//     the committee sum (near-full participation: a handful of additions
//     instead of ~500); otherwise the rows walk the participants.  Row q owns
//     members q, q + 32, ...: bit q of each word of the row, so the walk is
//     row-uniform;
//   * an exceptional addition on either side (duplicate members make P == +-Q
//     ordinary) leaves Z = 0, and ka_finish then sums the PARTICIPANTS on one
//     lane with the exact formulas -- never a one-lane complement; a sum that
//     is truly infinity fails the set.
// ---------------------------------------------------------------------------
#define KB_WORDS 64  // 2048 members
struct kb_set {
  ka_set a;
  uint32_t row[KB_WORDS];  // the bit row, then the walk mask
  uint32_t c, av, hit;
};

// bad[t]: bit j set when member 32 t + j's table key is not TB_SUCCESS (or its
// index is past the table); valid[t]: the in-range members that are not bad
extern "C" __global__ void __launch_bounds__(KB_WORDS)
    k_committee_mask(const uint32_t* __restrict__ members, uint32_t size, const uint8_t* __restrict__ tab_code, uint32_t tab_n,
                     uint32_t* __restrict__ bad, uint32_t* __restrict__ valid) {
  const uint32_t t = threadIdx.x;
  if (t >= KB_WORDS) return;
  uint32_t b = 0, in = 0;
  for (uint32_t j = 0; j < 32; j++) {
    const uint32_t m = 32 * t + j;
    if (m >= size) break;
    in |= 1u << j;
    const uint32_t k = members[m];
    if (k >= tab_n || tab_code[k] != TB_SUCCESS) b |= 1u << j;
  }
  bad[t] = b;
  valid[t] = in & ~b;
}

// the exact one-lane body of a bitfield set: the participants, in committee order
__device__ TB_NOINLINE int kb_set_generic(const uint32_t* row, const uint32_t* members, uint32_t size, const g1a* tab_aff,
                                          const uint8_t* tab_code, uint32_t tab_n, uint64_t r, g1a& o) {
  o.x = fp_zero();
  o.y = fp_zero();
  g1j acc = jac_inf<fp>();
  for (uint32_t j = 0; j < size; j++) {
    if (!((row[j >> 5] >> (j & 31u)) & 1u)) continue;
    const uint32_t k = members[j];
    if (k >= tab_n) return TB_BAD_ENCODING;
    if (tab_code[k] != TB_SUCCESS) return TB_PK_IS_INFINITY;  // BlstPublicKey.java:58-65
    acc = jac_add_aff(acc, tab_aff[k]);
  }
  return stage_set_pk_finish(acc, r, o);
}

// rows: n bit rows of stride_w words (>= ceil(size / 32); bits past size are
// ignored); csum / sum_ok: the committee sum and whether it may be used.
extern "C" __global__ void __launch_bounds__(KA_ROWS * 16)
    k_set_pk_bits_coop(const uint32_t* __restrict__ rows, uint32_t stride_w, const uint32_t* __restrict__ members, uint32_t size,
                       const uint32_t* __restrict__ bad, const g1a* __restrict__ csum, uint32_t sum_ok,
                       const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, uint32_t tab_n,
                       const uint64_t* __restrict__ rand, uint32_t n, g1a* __restrict__ P, uint8_t* __restrict__ set_code,
                       uint32_t* __restrict__ n_bad, g1a* __restrict__ P2, const g1a* __restrict__ comb, uint32_t unit_r) {
  __shared__ kb_set B;
  ka_set& S = B.a;
  tb_latency_prio();
  const int q = crow::row(), d = crow::dig();
  const coop::cctx K = coop::cctx_load();
  const c32 one = crow::from_const(R1);
  if (size > 32u * KB_WORDS) size = 32u * KB_WORDS;
  const uint32_t nw = std::min<uint32_t>((size + 31u) / 32u, stride_w);
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t* row = rows + (size_t)i * stride_w;
    const uint64_t rnd = unit_r ? 1ull : rand[i];
    if (threadIdx.x == 0) {
      S.bad = TB_SUCCESS;
      B.c = B.av = B.hit = 0u;
    }
    __syncthreads();
    // ---- the bit row: participants, absent valid members, participating bad members
    uint32_t wb = 0, wa = 0;
    if (threadIdx.x < nw) {
      const uint32_t t = threadIdx.x, left = size - 32u * t;
      const uint32_t in = left >= 32u ? 0xffffffffu : (1u << left) - 1u, bd = bad[t];
      wb = row[t] & in;
      wa = ~wb & ~bd & in;
      atomicAdd(&B.c, (uint32_t)__popc(wb));
      atomicAdd(&B.av, (uint32_t)__popc(wa));
      if (wb & bd) atomicOr(&B.hit, 1u);
      wb &= ~bd;
    }
    __syncthreads();
    const bool comp = sum_ok != 0u && B.av < B.c;  // the cheaper side
    if (threadIdx.x < nw) B.row[threadIdx.x] = comp ? wa : wb;
    if (threadIdx.x == 0 && B.hit) S.bad = TB_PK_IS_INFINITY;  // BlstPublicKey.java:58-65
    __syncthreads();
    // ---- row sums over the chosen side (row-uniform: bit q of every word)
    coop::cj1 acc = {c32(0), c32(0), c32(0)};
    bool inf = true;
    for (uint32_t t = 0; t < nw; t++) {
      if (!((B.row[t] >> q) & 1u)) continue;
      const uint32_t k = members[32u * t + (uint32_t)q];
      if (k >= tab_n) {
        S.bad = TB_BAD_ENCODING;
        continue;
      }
      const c32 qx = crow::from_fp(tab_aff[k].x), y = crow::from_fp(tab_aff[k].y);
      const c32 qy = comp ? -y : y;
      if (inf) {
        acc = {qx, qy, one};
        inf = false;
      } else {
        acc = coop::madd(acc, qx, qy, K);
      }
    }
    S.pt[q][0][d] = acc.x;
    S.pt[q][1][d] = acc.y;
    S.pt[q][2][d] = acc.z;
    if (d == 0) S.inf[q] = inf ? 1u : 0u;
    __syncthreads();
    ka_tree(S, KA_ROWS, q, d, K);
    if (comp && q == 0) {  // the committee sum minus the absent members
      const c32 sx = crow::from_fp(csum->x), sy = crow::from_fp(csum->y);
      coop::cj1 m = {sx, sy, one};
      if (S.inf[0] == 0) {
        const coop::cj1 neg = {S.pt[0][0][d], S.pt[0][1][d], S.pt[0][2][d]};
        m = coop::madd(neg, sx, sy, K);
      }
      __builtin_amdgcn_wave_barrier();  // every lane of the row has read inf[0]
      S.pt[0][0][d] = m.x;
      S.pt[0][1][d] = m.y;
      S.pt[0][2][d] = m.z;
      if (d == 0) S.inf[0] = 0u;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    ka_finish(S, i, rnd, rand, P, P2, set_code, n_bad, comb, q, d, K, one, [&](uint64_t r, g1a& o) {
      return kb_set_generic(row, members, size, tab_aff, tab_code, tab_n, r, o);
    });
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Grouped batches (tb_group.h, DESIGN.md "Grouped batches"): the sets that
// sign one message share one main pair (sum_{i in g} [r_i] apk_i, H(m_g)).
// The key stage leaves the sets' [r_i] apk_i in a per-set array; these kernels
// sum them per group, over the CSR (grp_off, grp_sets), in the layout of
// k_set_pk_agg_coop: one 512-thread workgroup per sum, row q walks members q,
// q + 32, ... with coop mixed additions, the 32 row sums meet in the LDS row
// tree (ka_tree) and lane 0 of row 0 inverts once (ka_affine).
//   * Members whose code is nonzero (an invalid set: its point is undefined)
//     are left out; the set already counts in n_bad, which decides the verdict.
//   * The coop additions have no exceptional-case branches, and here P == +-Q
//     is ordinary input (one key twice under one message with equal
//     randomizers; a key and its negation): such a sum ends with Z = 0, and
//     lane 0 then sums the members again with the exact formulas
//     (gs_exact).  A sum that is truly infinity, or has no member left, gets
//     its flag set: e(inf, H) = 1, the pair is skipped and nothing has failed.
//   * A sum of one member is a copy: no tree, no inversion.
//   * A group of more than `walk` members (tb_plan.h group_walk) is split
//     into items of `walk` members: k_group_items numbers the items
//     (item_first[g]: group g's first), pass 0 writes the items' sums to
//     part / part_skip (straight to PG / pskip for a group of one item) and
//     pass 1 sums the items of every split group the same way.
// Offsets and indices come from the caller of the device entry: they are
// clamped to the arrays (n members, items_max items), never trusted.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
    k_group_items(const uint32_t* __restrict__ grp_off, uint32_t m, uint32_t n, uint32_t walk, uint32_t* __restrict__ item_first) {
  __shared__ uint32_t part[256];
  const uint32_t t = threadIdx.x, per = (m + 255u) / 256u, lo = std::min(m, t * per), hi = std::min(m, lo + per);
  const auto items = [&](uint32_t g) {
    const uint32_t e = std::min(grp_off[g + 1], n), b = std::min(grp_off[g], e), c = e - b;
    return c ? (c + walk - 1u) / walk : 1u;
  };
  uint32_t sum = 0;
  for (uint32_t g = lo; g < hi; g++) sum += items(g);
  part[t] = sum;
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t k = 0; k < t; k++) base += part[k];
  for (uint32_t g = lo; g < hi; g++) {
    item_first[g] = base;
    base += items(g);
  }
  if (t == 255u) item_first[m] = base;  // the last thread's range ends at m: the total
}

// the exact sum of members [lo, hi) on one lane; false: infinity
__device__ TB_NOINLINE bool gs_exact(const g1a* __restrict__ pts, const uint8_t* __restrict__ code, const uint32_t* __restrict__ list,
                                     uint32_t n_pts, uint32_t lo, uint32_t hi, g1a& o) {
  g1j acc = jac_inf<fp>();
  for (uint32_t j = lo; j < hi; j++) {
    const uint32_t k = list ? list[j] : j;
    if (k < n_pts && code[k] == 0) acc = jac_add_aff(acc, pts[k]);
  }
  return jac_to_aff(o, acc);
}

// out / oskip: the sum of pts[list[j]] (list nullptr: pts[j]) over lo <= j < hi with code 0 (all threads call)
__device__ TB_INLINE void gs_sum(ka_set& S, const g1a* __restrict__ pts, const uint8_t* __restrict__ code, const uint32_t* __restrict__ list,
                                 uint32_t n_pts, uint32_t lo, uint32_t hi, g1a* __restrict__ out, uint8_t* __restrict__ oskip, int q, int d,
                                 const coop::cctx& K, const c32& one) {
  if (hi <= lo + 1u) {  // no member, or one: a copy
    if (threadIdx.x == 0) {
      g1a o;
      o.x = fp_zero();
      o.y = fp_zero();
      uint8_t sk = 1;
      if (hi > lo) {
        const uint32_t k = list ? list[lo] : lo;
        if (k < n_pts && code[k] == 0) {
          o = pts[k];
          sk = 0;
        }
      }
      *out = o;
      *oskip = sk;
    }
    return;
  }
  coop::cj1 acc = {c32(0), c32(0), c32(0)};
  bool inf = true;
  for (uint32_t j = lo + (uint32_t)q; j < hi; j += KA_ROWS) {
    const uint32_t k = list ? list[j] : j;
    if (k >= n_pts || code[k] != 0) continue;
    const c32 qx = crow::from_fp(pts[k].x), qy = crow::from_fp(pts[k].y);
    if (inf) {
      acc = {qx, qy, one};
      inf = false;
    } else {
      acc = coop::madd(acc, qx, qy, K);
    }
  }
  S.pt[q][0][d] = acc.x;
  S.pt[q][1][d] = acc.y;
  S.pt[q][2][d] = acc.z;
  if (d == 0) S.inf[q] = inf ? 1u : 0u;
  __syncthreads();
  ka_tree(S, KA_ROWS, q, d, K);
  if (q == 0) {  // 0: the coop sum stands, 1: exceptional -> the exact body, 2: no member left
    const c32 zv[1] = {S.pt[0][2][d]};
    const bool zero = crow::zeros_n<1>(zv, S.zb[0]) != 0u;
    if (d == 0) S.mode = S.inf[0] != 0 ? 2 : zero ? 1 : 0;
  }
  __syncthreads();
  const int mode = S.mode;
  if (q == 0) {
    if (mode == 0) {
      const coop::cj1 rp = {S.pt[0][0][d], S.pt[0][1][d], S.pt[0][2][d]};
      ka_affine(rp, S.zb[0], S.inv[0], S.out[0], d, K);
    }
    if (d == 0) {
      g1a o;
      o.x = fp_zero();
      o.y = fp_zero();
      uint8_t sk = 1;
      if (mode == 0) {
        o.x = S.out[0][0];
        o.y = S.out[0][1];
        sk = 0;
      } else if (mode == 1) {
        g1a e;
        if (gs_exact(pts, code, list, n_pts, lo, hi, e)) {
          o = e;
          sk = 0;
        }
      }
      *out = o;
      *oskip = sk;
    }
  }
  __syncthreads();  // S is free for the next sum
}

// pass 0: the items of every group, from the sets' points (pts, code: n of
// them) over the CSR; pass 1: the split groups, from their items' sums (part,
// part_skip).  item_first nullptr: no group is split (item g = group g).
extern "C" __global__ void __launch_bounds__(KA_ROWS * 16)
    k_group_pk_sum_coop(const g1a* __restrict__ pts, const uint8_t* __restrict__ code, uint32_t n, const uint32_t* __restrict__ grp_off,
                        const uint32_t* __restrict__ grp_sets, const uint32_t* __restrict__ item_first, uint32_t m, uint32_t walk,
                        uint32_t items_max, uint32_t pass, g1a* __restrict__ PG, uint8_t* __restrict__ pskip, g1a* __restrict__ part,
                        uint8_t* __restrict__ part_skip) {
  __shared__ ka_set S;
  tb_latency_prio();
  const int q = crow::row(), d = crow::dig();
  const coop::cctx K = coop::cctx_load();
  const c32 one = crow::from_const(R1);
  if (pass == 0) {
    const uint32_t total = item_first ? std::min(item_first[m], items_max) : m;
    for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
      uint32_t g = w, k = 0, single = 1;
      if (item_first) {  // the last group whose first item is <= w
        uint32_t a = 0, b = m;
        while (b - a > 1u) {
          const uint32_t c = (a + b) / 2u;
          if (item_first[c] <= w) a = c;
          else b = c;
        }
        g = a;
        k = w - item_first[g];
        single = item_first[g + 1] - item_first[g] == 1u;
      }
      const uint32_t e = std::min(grp_off[g + 1], n), b0 = std::min(grp_off[g], e);
      const uint32_t lo = std::min(e, b0 + k * walk), hi = item_first ? std::min(e, lo + walk) : e;
      gs_sum(S, pts, code, grp_sets, n, lo, hi, single ? PG + g : part + w, single ? pskip + g : part_skip + w, q, d, K, one);
    }
  } else {
    for (uint32_t g = blockIdx.x; g < m; g += gridDim.x) {
      const uint32_t a = std::min(item_first[g], items_max), b = std::min(item_first[g + 1], items_max);
      if (b - a < 2u) continue;
      gs_sum(S, part, part_skip, nullptr, items_max, a, b, PG + g, pskip + g, q, d, K, one);
    }
  }
}
