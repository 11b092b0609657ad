// The hash-point memo's two kernels (tb_msgmemo.h): both move
// affine G2 points (192 bytes) with their skip byte between the batch's hashed
// points Qh, the device's resident rows and the main pairs' Q, by indices the
// host resolved before launch.  Copy kernels: one thread per 16-byte chunk, 12
// threads per point, uint4 loads and stores, so a wave reads and writes whole
// cache lines of consecutive points; 256-thread workgroups with a handful of
// registers, no LDS, no scratch, no atomics.  Every array of points is 16-byte
// aligned by layout (tb_plan.h ws_layout; the rows: tb_lib.hip memo_rows).
#include "tb_kdecl.h"

using namespace tb;

static_assert(sizeof(g2a) == 16 * TB_MEMO_CHUNKS, "a point is copied as twelve 16-byte words");

// Q[i], skip[i] for every main pair i < n_pairs: its group is set_grp[i] (an
// ungrouped pass: i is a set) or i itself (set_grp null: a grouped pass), and
// the group's word src[g] names row r (TB_MEMO_SRC_ROW | r) or hashed point j.
extern "C" __global__ void __launch_bounds__(TB_MEMO_BLOCK)
    k_memo_fill(const uint32_t* __restrict__ src, const uint32_t* __restrict__ set_grp, uint32_t n_pairs, const g2a* __restrict__ Qh,
                const uint8_t* __restrict__ skiph, const g2a* __restrict__ rows, const uint8_t* __restrict__ row_skip, g2a* __restrict__ Q,
                uint8_t* __restrict__ skip) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = t / TB_MEMO_CHUNKS, k = t % TB_MEMO_CHUNKS;
  if (i >= n_pairs) return;
  const uint32_t w = src[set_grp ? set_grp[i] : i];
  const bool row = (w & TB_MEMO_SRC_ROW) != 0;
  const uint32_t e = w & ~TB_MEMO_SRC_ROW;
  const uint4* from = reinterpret_cast<const uint4*>(row ? rows + e : Qh + e);
  reinterpret_cast<uint4*>(Q + i)[k] = from[k];
  if (k == 0) skip[i] = row ? row_skip[e] : skiph[e];
}

// rows[learn[j]], row_skip[learn[j]] = Qh[j], skiph[j] for every hashed
// message j < m_hash whose learn word is not TB_MEMO_NONE.  The values are the
// final ones (behind k_set_hash_fix), so a stored skip byte is 0 or 1.
extern "C" __global__ void __launch_bounds__(TB_MEMO_BLOCK)
    k_memo_learn(const uint32_t* __restrict__ learn, uint32_t m_hash, const g2a* __restrict__ Qh, const uint8_t* __restrict__ skiph,
                 g2a* __restrict__ rows, uint8_t* __restrict__ row_skip) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t j = t / TB_MEMO_CHUNKS, k = t % TB_MEMO_CHUNKS;
  if (j >= m_hash) return;
  const uint32_t r = learn[j];
  if (r == TB_MEMO_NONE) return;
  reinterpret_cast<uint4*>(rows + r)[k] = reinterpret_cast<const uint4*>(Qh + j)[k];
  if (k == 0) row_skip[r] = skiph[j];
}
