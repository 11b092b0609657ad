// Settling a failed grouped batch from the grouped pass's own work (tb_lib.hip
// settle_grouped).  Set i's randomized Miller value is
//   f([r_i] apk_i, H(m_g(i))) * f(-[r_i] g1, sig_i).
// The split Miller loop stores lines already evaluated at the pair's G1 point
// (tb_lines.h: l.b carries P.x, l.c carries P.y), so a group's line table
// cannot serve its members as it stands.  Here:
//   k_gsettle_msg_lines      the 68 lines of each H(m_g), evaluated at the unit
//                            point (Montgomery one for x and y: the two
//                            scalings leave the coefficients as they are), one
//                            column per message, stored without the
//                            non-temporal hint: every member of the group
//                            reads its message's column again;
//   k_gsettle_prep           per position t of the CSR (set grp_sets[t]): its
//                            message, and for one chunk of positions the line
//                            kernel's inputs in position order -- -[r] g1 from
//                            the comb table, the decoded signature, and the
//                            skip flag;
//   (the chunk's signature lines: an existing line kernel, tb_lib.hip)
//   k_miller_accs_gsettle    the LDS-resident segmented accumulator of
//                            k_miller_accs_lds with another line source: line
//                            1 from the message table, its b scaled by
//                            set_P[i].x and its c by set_P[i].y on load (4 Fp
//                            products), line 2 from the chunk's signature
//                            table at the position's column.
// Positions, not set indices, so that adjacent lanes share a message and a
// wave's message-line loads are mostly to one address.
#include "tb_comb.h"
#include "tb_lines.h"

using namespace tb;

namespace {
// line s of message g in the table of m columns (tb_lines.h line_store's layout, plain stores)
__device__ TB_INLINE void msg_line_store(uint4* __restrict__ lines, uint32_t m, uint32_t g, int s, const line3& l) {
  const fp* c[6] = {&l.a.c0, &l.a.c1, &l.b.c0, &l.b.c1, &l.c.c0, &l.c.c1};
  TB_UNROLL for (int k = 0; k < TB_LINE_G; k++) {
    const int w = 4 * k;
    uint4 v;
    v.x = c[(w + 0) / 12]->l[(w + 0) % 12];
    v.y = c[(w + 1) / 12]->l[(w + 1) % 12];
    v.z = c[(w + 2) / 12]->l[(w + 2) % 12];
    v.w = c[(w + 3) / 12]->l[(w + 3) % 12];
    lines[(size_t)(s * TB_LINE_G + k) * m + g] = v;
  }
}

// the same line, b scaled by P.x and c by P.y
__device__ TB_INLINE line3 msg_line_load(const uint4* __restrict__ lines, uint32_t m, uint32_t g, int s, const g1a& P) {
  line3 l;
  fp* c[6] = {&l.a.c0, &l.a.c1, &l.b.c0, &l.b.c1, &l.c.c0, &l.c.c1};
  const uint4* __restrict__ row = lines + (size_t)(s * TB_LINE_G) * m;
  TB_UNROLL for (int k = 0; k < TB_LINE_G; k++) {
    const uint4 v = row[(size_t)k * m + g];
    const int w = 4 * k;
    c[(w + 0) / 12]->l[(w + 0) % 12] = v.x;
    c[(w + 1) / 12]->l[(w + 1) % 12] = v.y;
    c[(w + 2) / 12]->l[(w + 2) % 12] = v.z;
    c[(w + 3) / 12]->l[(w + 3) % 12] = v.w;
  }
  l.b = mf(l.b, P.x);
  l.c = mf(l.c, P.y);
  return l;
}
}  // namespace

// One thread per message: the lines of H(m_g) at the unit point.  A message
// with skip[g] != 0 gets no lines (the accumulator never reads its column).
extern "C" __global__ void __launch_bounds__(TB_BLOCK, 1)
    k_gsettle_msg_lines(const g2a* __restrict__ Q, const uint8_t* __restrict__ skip, uint32_t m, uint4* __restrict__ lines) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= m || skip[g] != 0) return;
  const g1a unit = {fp_one(), fp_one()};
  const g2a q = Q[g];
  g2p T = {q.x, q.y, fp2_one()};
  int s = 0;
  TB_NOUNROLL for (int b = 62; b >= 0; --b) {
    msg_line_store(lines, m, g, s++, dbl_step_f(T, unit));
    if ((X_ABS >> b) & 1) msg_line_store(lines, m, g, s++, add_step_f(T, q, unit));
  }
}

// Positions [lo, lo + cn) of the CSR (n positions, m groups): msg_of_pos[t],
// and in chunk order (k = t - lo) the signature pair of set i = grp_sets[t]:
// negr[k] = -[r_i] g1, sigq[k] = sig_aff[i], sskip[k] != 0 when the pair
// contributes 1 -- the set is invalid by its codes, its message is skipped, or
// its signature is the (valid) point at infinity.
extern "C" __global__ void __launch_bounds__(TB_BLOCK)
    k_gsettle_prep(const uint32_t* __restrict__ grp_off, const uint32_t* __restrict__ grp_sets, uint32_t m, uint32_t n, uint32_t lo, uint32_t cn,
                   const uint64_t* __restrict__ rand, const g1a* __restrict__ comb, const g2a* __restrict__ sig_aff,
                   const uint8_t* __restrict__ sig_use, const uint8_t* __restrict__ set_code, const uint8_t* __restrict__ sig_code,
                   const uint8_t* __restrict__ msg_skip, uint32_t* __restrict__ msg_of_pos, g1a* __restrict__ negr, g2a* __restrict__ sigq,
                   uint8_t* __restrict__ sskip) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cn || lo + k >= n) return;
  const uint32_t t = lo + k;
  // the group with grp_off[g] <= t < grp_off[g + 1] (empty groups do not occur)
  uint32_t a = 0, b = m;
  while (b - a > 1) {
    const uint32_t mid = a + (b - a) / 2;
    if (grp_off[mid] <= t)
      a = mid;
    else
      b = mid;
  }
  msg_of_pos[t] = a;
  const uint32_t i = grp_sets[t];
  const bool dead = i >= n || set_code[i] != 0 || sig_code[i] != 0 || msg_skip[a] != 0;
  const bool use = !dead && sig_use[i] != 0;
  sskip[k] = use ? 0 : 1;
  if (!use) return;
  negr[k] = neg_r_g1(comb, rand[i]);
  sigq[k] = sig_aff[i];
}

// Segment j of position lo + k (k < cn) to V[j * n + lo + k]; the grid is nseg
// x g_pad / TB_BLOCK workgroups as k_miller_accs_lds's, g_pad >= cn a multiple
// of the block.  mlines: m columns; slines: the chunk's cn columns.
extern "C" __global__ void __launch_bounds__(TB_BLOCK, 1)
    k_miller_accs_gsettle(const uint4* __restrict__ mlines, uint32_t m, const uint32_t* __restrict__ msg_of_pos,
                          const uint32_t* __restrict__ grp_sets, const g1a* __restrict__ set_P, const uint8_t* __restrict__ set_code,
                          const uint8_t* __restrict__ sig_code, const uint8_t* __restrict__ msg_skip, const uint4* __restrict__ slines,
                          const uint8_t* __restrict__ sskip, uint32_t lo, uint32_t cn, uint32_t n, uint32_t nseg, uint32_t g_pad,
                          fp12* __restrict__ V) {
  __shared__ uint4 Fsh[36 * TB_BLOCK];
  const uint32_t bps = g_pad / TB_BLOCK;
  const uint32_t j = blockIdx.x / bps, k = (blockIdx.x % bps) * TB_BLOCK + threadIdx.x;
  if (j >= nseg || k >= cn || lo + k >= n) return;
  const uint32_t t = lo + k;
  fp12* out = V + (size_t)j * n + t;
  const uint32_t i = grp_sets[t], g = msg_of_pos[t];
  if (i >= n || g >= m || set_code[i] != 0 || sig_code[i] != 0 || msg_skip[g] != 0) {  // the verdict comes from the code
    *out = fp12_one();
    return;
  }
  const bool two = sskip[k] == 0;
  const g1a P = set_P[i];
  const int s_lo = (int)(TB_LINE_STEPS * j / nseg), s_hi = (int)(TB_LINE_STEPS * (j + 1) / nseg);
  const lds12 F{Fsh + threadIdx.x, 0};
  bool fresh = true;  // f == 1 (not yet written)
  TB_NOUNROLL for (int s = s_lo; s < s_hi; s++) {
    if (!fresh && step_is_dbl(s)) fp12_sqr_lds(F);
    const line3 l1 = msg_line_load(mlines, m, g, s, P);
    if (two) {
      const line2 L = line_mul(l1, line_load(slines, cn, k, s));
      if (fresh) {
        F.st6(0, L.x);
        F.st6(1, {fp2_zero(), L.y1, L.y2});
        fresh = false;
      } else if (TB_ACC_LINE2 == 2) {
        fp12_mul_line2_lds_s1(F, L);
      } else {
        fp12_mul_line2_lds(F, L);
      }
    } else if (fresh) {
      F.st6(0, {l1.a, l1.b, fp2_zero()});
      F.st6(1, {fp2_zero(), l1.c, fp2_zero()});
      fresh = false;
    } else {
      fp12_mul_line_lds(F, l1);
    }
  }
  const fp12 f = fresh ? fp12_one() : fp12{F.ld6(0), F.ld6(1)};
  *out = fp12_conj(f);
}
