// Byte-level hook of the hash-point memo's kernels (teku_amd/csrc/k_msgmemo.hip).
// TEST INFRASTRUCTURE (libtekubls_test.so; never loaded by the product): like
// k_test_stages.hip it launches the PRODUCT library's own k_memo_fill and
// k_memo_learn -- looked up by name in the already-loaded libtekubls_hip.so --
// with the grid and block of tb_lib.hip (memo_grid: 12 threads per point,
// 256-thread workgroups) on caller byte arrays, and returns the arrays they
// wrote for tests/test_gpu_msgmemo_kernels.py to compare with a numpy gather.
//
// tbls_test_memo(product_so, src, n_groups, set_grp (nullable), n_pairs,
//                qh, skiph, m_hash, learn, rows, row_skip, n_rows, pad,
//                q_io, skip_io):
//   qh / skiph       m_hash x 192 / m_hash bytes: the "hashed" points
//   rows / row_skip  n_rows x 192 / n_rows bytes, in and out: k_memo_fill reads
//                    them as given, then k_memo_learn writes the rows that
//                    learn names, and the result comes back
//   q_io / skip_io   (n_pairs + pad) x 192 / n_pairs + pad bytes, in and out:
//                    the caller's preset bytes, of which k_memo_fill may write
//                    the first n_pairs entries only
// The hook checks every index against its array before anything is launched
// (-1), so a bad case cannot read or write out of bounds on the device.
// Every HIP status is checked: the first failure returns a negative code and
// nothing more is launched.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
constexpr uint32_t BLOCK = 256, CHUNKS = 12, SRC_ROW = 0x80000000u, NONE = 0xffffffffu;  // TB_MEMO_* (tb_kdecl.h)
constexpr size_t PT = 192;                                                                // sizeof(g2a)

struct dev_mem {
  void* p = nullptr;
  ~dev_mem() {
    if (p) (void)hipFree(p);
  }
  int put(const void* src, size_t n) {
    if (hipMalloc(&p, n ? n : 1) != hipSuccess) return -1;
    return n && hipMemcpy(p, src, n, hipMemcpyHostToDevice) != hipSuccess ? -1 : 0;
  }
  int get(void* dst, size_t n) const { return !n || hipMemcpy(dst, p, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
};

int launch(void* fn, uint32_t points, void** args) {
  if (!fn) return -2;
  const uint32_t grid = (uint32_t)(((uint64_t)points * CHUNKS + BLOCK - 1) / BLOCK);
  return hipLaunchKernel(fn, dim3(grid), dim3(BLOCK), args, 0, nullptr) == hipSuccess ? 0 : -3;
}
}  // namespace

extern "C" int tbls_test_memo(const char* product_so, const uint32_t* src, uint32_t n_groups, const uint32_t* set_grp, uint32_t n_pairs,
                              const uint8_t* qh, const uint8_t* skiph, uint32_t m_hash, const uint32_t* learn, uint8_t* rows, uint8_t* row_skip,
                              uint32_t n_rows, uint32_t pad, uint8_t* q_io, uint8_t* skip_io) {
  if (!n_pairs || !n_groups || (!set_grp && n_groups < n_pairs)) return -1;
  for (uint32_t i = 0; set_grp && i < n_pairs; i++)
    if (set_grp[i] >= n_groups) return -1;
  for (uint32_t g = 0; g < n_groups; g++)
    if ((src[g] & SRC_ROW) ? (src[g] & ~SRC_ROW) >= n_rows : src[g] >= m_hash) return -1;
  for (uint32_t j = 0; j < m_hash; j++)
    if (learn[j] != NONE && learn[j] >= n_rows) return -1;
  void* h = dlopen(product_so, RTLD_NOW | RTLD_NOLOAD);  // the instance the tests already use
  if (!h) h = dlopen(product_so, RTLD_NOW);
  if (!h) return -4;
  const size_t nq = (size_t)n_pairs + pad;
  dev_mem dsrc, dgrp, dqh, dsh, dlearn, drows, drs, dq, dskip;
  if (dsrc.put(src, 4 * (size_t)n_groups) || (set_grp && dgrp.put(set_grp, 4 * (size_t)n_pairs)) || dqh.put(qh, PT * m_hash) ||
      dsh.put(skiph, m_hash) || dlearn.put(learn, 4 * (size_t)m_hash) || drows.put(rows, PT * n_rows) || drs.put(row_skip, n_rows) ||
      dq.put(q_io, PT * nq) || dskip.put(skip_io, nq))
    return -6;
  {
    void* a[] = {&dsrc.p, &dgrp.p, &n_pairs, &dqh.p, &dsh.p, &drows.p, &drs.p, &dq.p, &dskip.p};
    if (const int rc = launch(dlsym(h, "k_memo_fill"), n_pairs, a)) return rc;
  }
  if (m_hash) {
    void* a[] = {&dlearn.p, &m_hash, &dqh.p, &dsh.p, &drows.p, &drs.p};
    if (const int rc = launch(dlsym(h, "k_memo_learn"), m_hash, a)) return rc;
  }
  if (hipDeviceSynchronize() != hipSuccess) return -7;
  return dq.get(q_io, PT * nq) || dskip.get(skip_io, nq) || drows.get(rows, PT * n_rows) || drs.get(row_skip, n_rows) ? -8 : 0;
}
