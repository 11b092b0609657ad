// Byte-level parity hook of the Miller stage: the line kernels, the
// accumulators, the Fp12 products, the segment combine, the group test and the
// settle kernels.
// TEST INFRASTRUCTURE (libtekubls_test.so; never loaded by the product): like
// k_test_stages.hip it launches the PRODUCT library's own kernels -- looked up
// by name in the already-loaded libtekubls_hip.so -- with the grids and blocks
// of tb_lib.hip (partial_run::miller, product_tree, settle_sets, settle_tail,
// settle_grouped, group_tests) and the argument lists of tb_kdecl.h, on caller
// inputs, and returns their raw outputs for tests/test_gpu_pair_stage.py to
// compare with tests/pair_cases.py.
//
// Every output buffer is preset to 0xEE (an unwritten slot shows) and is
// followed by GUARD bytes of 0xEE, which come back behind the payload: an
// `out` pointer of `size` payload bytes receives size + GUARD bytes.  GUARD
// is 64 Fp12 values: the padded lanes [G, g_pad) of an accumulator's last
// segment would write there.  Every allocation is sized from the launch
// arguments, and a shape whose reads would pass an input buffer is refused
// (-1) before anything is launched.  Every HIP status is checked: the first
// failure returns a negative code and nothing more is launched.
//
//   tbls_test_pair_guard       GUARD
//   tbls_test_pair_lines       variant 0 k_miller_lines_w2, 1 k_miller_lines_quad,
//                              2 k_miller_lines_duo -> the line table, 68 * 18 * n 16-byte words
//   tbls_test_pair_msg_lines   k_gsettle_msg_lines -> 68 * 18 * m words
//   tbls_test_pair_acc         variant 0 k_miller_acc1, 1 k_miller_acc2 (per and nseg ignored),
//                              2 k_miller_accs_lds -> f_out, nseg * G values, seg_stride = G = ceil(n / per)
//   tbls_test_pair_accs_gsettle  k_miller_accs_gsettle -> V, nseg * n values
//   tbls_test_pair_gsettle_prep  k_g1_comb_init + k_gsettle_prep -> msg_of_pos n words, negr cn g1a, sigq cn g2a, sskip cn
//   tbls_test_pair_prod        k_fp12_prod_wave on a grid of `grid` workgroups -> grid values
//   tbls_test_pair_prod_seg    k_fp12_prod_wave_seg, grid (grid_x, nseg) -> (nseg - 1) * out_stride + grid_x values
//   tbls_test_pair_combine     k_fp12_seg_combine_coop -> one value
//   tbls_test_pair_group_test  k_group_test_coop -> n_list bytes
//   tbls_test_pair_miller_wave k_miller_wave -> n values
//   tbls_test_pair_settle_mask k_settle_mask on the caller's 2n skip bytes -> 2n bytes
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../teku_amd/csrc/tb_plan.h"

namespace {
constexpr uint32_t BLK = 64;         // TB_BLOCK (tb_kdecl.h)
constexpr uint32_t COOP = 256;       // TB_CFE_THREADS (tb_kdecl.h)
constexpr size_t F12 = sizeof(tb::fp12);
constexpr size_t GUARD = 64 * F12;
constexpr size_t LINE_WORDS = 68 * 18;  // 16-byte words of a pair's lines (tb_lines.h)
static_assert(F12 == 576 && sizeof(tb::g1a) == 96 && sizeof(tb::g2a) == 192, "the sizes tests/pair_cases.py decodes");

struct dev_mem {
  void* p = nullptr;
  size_t size = 0;
  ~dev_mem() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t n) {
    size = n;
    return hipMalloc(&p, n ? n : 1) == hipSuccess ? 0 : -1;
  }
  int put(const void* src, size_t n) { return alloc(n) || (n && hipMemcpy(p, src, n, hipMemcpyHostToDevice) != hipSuccess) ? -1 : 0; }
  // an output of n payload bytes and the guard behind it, all 0xEE
  int out(size_t n) { return alloc(n + GUARD) || hipMemset(p, 0xee, n + GUARD) != hipSuccess ? -1 : 0; }
  int get(void* dst) const { return hipMemcpy(dst, p, size, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
};

int launch(void* fn, dim3 grid, uint32_t block, void** args) {
  if (!fn) return -2;
  return hipLaunchKernel(fn, grid, dim3(block), args, 0, nullptr) == hipSuccess ? 0 : -3;
}

void* product(const char* so) {
  void* h = dlopen(so, RTLD_NOW | RTLD_NOLOAD);  // the instance the tests already use
  return h ? h : dlopen(so, RTLD_NOW);
}

int finish(int rc) {
  if (rc) return rc;
  return hipDeviceSynchronize() == hipSuccess ? 0 : -7;
}

uint32_t pad(uint32_t n) { return (n + BLK - 1) / BLK * BLK; }
}  // namespace

extern "C" size_t tbls_test_pair_guard(void) { return GUARD; }

extern "C" int tbls_test_pair_lines(const char* product_so, int variant, const uint8_t* P, const uint8_t* Q, const uint8_t* skip,
                                    const uint8_t* code_a, const uint8_t* code_b, uint32_t n, uint8_t* lines_out) {
  if (n == 0 || variant < 0 || variant > 2) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem dP, dQ, ds, da, db, dl;
  if (dP.put(P, n * sizeof(tb::g1a)) || dQ.put(Q, n * sizeof(tb::g2a)) || ds.put(skip, n) || da.put(code_a, n) || db.put(code_b, n)) return -6;
  if (dl.out(LINE_WORDS * n * 16)) return -5;
  const uint32_t lg = variant == 1 ? 4u : variant == 2 ? 2u : 1u;  // lanes per pair (tb_lib.hip line_kernel_of)
  void* a[] = {&dP.p, &dQ.p, &ds.p, &da.p, &db.p, &n, &dl.p};
  const char* name = variant == 1 ? "k_miller_lines_quad" : variant == 2 ? "k_miller_lines_duo" : "k_miller_lines_w2";
  if (const int rc = finish(launch(dlsym(h, name), dim3((lg * n + BLK - 1) / BLK), BLK, a))) return rc;
  return dl.get(lines_out) ? -8 : 0;
}

extern "C" int tbls_test_pair_msg_lines(const char* product_so, const uint8_t* Q, const uint8_t* skip, uint32_t m, uint8_t* lines_out) {
  if (m == 0) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem dQ, ds, dl;
  if (dQ.put(Q, m * sizeof(tb::g2a)) || ds.put(skip, m)) return -6;
  if (dl.out(LINE_WORDS * m * 16)) return -5;
  void* a[] = {&dQ.p, &ds.p, &m, &dl.p};
  if (const int rc = finish(launch(dlsym(h, "k_gsettle_msg_lines"), dim3((m + BLK - 1) / BLK), BLK, a))) return rc;
  return dl.get(lines_out) ? -8 : 0;
}

extern "C" int tbls_test_pair_acc(const char* product_so, int variant, const uint8_t* lines, const uint8_t* skip, const uint8_t* code_a,
                                  const uint8_t* code_b, uint32_t n, uint32_t per, uint32_t nseg, uint8_t* f_out) {
  if (variant == 0) per = 1, nseg = 1;
  if (variant == 1) per = 2, nseg = 1;
  if (n == 0 || variant < 0 || variant > 2 || per == 0 || per > 32 || nseg == 0 || nseg > 68) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem dl, ds, da, db, df;
  if (dl.put(lines, LINE_WORDS * n * 16) || ds.put(skip, n) || da.put(code_a, n) || db.put(code_b, n)) return -6;
  uint32_t G = (n + per - 1) / per, g_pad = pad(G);
  if (df.out((size_t)nseg * G * F12)) return -5;
  int rc;
  if (variant == 2) {  // partial_run::miller / settle_sets
    void* a[] = {&dl.p, &ds.p, &da.p, &db.p, &n, &per, &nseg, &g_pad, &df.p, &G};
    rc = launch(dlsym(h, "k_miller_accs_lds"), dim3(nseg * g_pad / BLK), BLK, a);
  } else {
    void* a[] = {&dl.p, &ds.p, &da.p, &db.p, &n, &df.p};
    rc = launch(dlsym(h, variant == 1 ? "k_miller_acc2" : "k_miller_acc1"), dim3((G + BLK - 1) / BLK), BLK, a);
  }
  if ((rc = finish(rc))) return rc;
  return df.get(f_out) ? -8 : 0;
}

extern "C" int tbls_test_pair_accs_gsettle(const char* product_so, const uint8_t* mlines, uint32_t m, const uint32_t* msg_of_pos,
                                           const uint32_t* grp_sets, const uint8_t* set_P, const uint8_t* set_code, const uint8_t* sig_code,
                                           const uint8_t* msg_skip, const uint8_t* slines, const uint8_t* sskip, uint32_t lo, uint32_t cn,
                                           uint32_t n, uint32_t nseg, uint8_t* v_out) {
  if (n == 0 || m == 0 || cn == 0 || nseg == 0 || nseg > 68 || lo >= n || cn > n - lo) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem dm, dmp, dgs, dP, dsc, dgc, dms, dsl, dsk, dV;
  if (dm.put(mlines, LINE_WORDS * m * 16) || dmp.put(msg_of_pos, 4 * (size_t)n) || dgs.put(grp_sets, 4 * (size_t)n) ||
      dP.put(set_P, n * sizeof(tb::g1a)) || dsc.put(set_code, n) || dgc.put(sig_code, n) || dms.put(msg_skip, m) ||
      dsl.put(slines, LINE_WORDS * cn * 16) || dsk.put(sskip, cn))
    return -6;
  if (dV.out((size_t)nseg * n * F12)) return -5;
  uint32_t g_pad = pad(cn);
  void* a[] = {&dm.p, &m, &dmp.p, &dgs.p, &dP.p, &dsc.p, &dgc.p, &dms.p, &dsl.p, &dsk.p, &lo, &cn, &n, &nseg, &g_pad, &dV.p};
  if (const int rc = finish(launch(dlsym(h, "k_miller_accs_gsettle"), dim3(nseg * g_pad / BLK), BLK, a))) return rc;
  return dV.get(v_out) ? -8 : 0;
}

extern "C" int tbls_test_pair_gsettle_prep(const char* product_so, const uint32_t* grp_off /* m + 1 */, const uint32_t* grp_sets, uint32_t m,
                                           uint32_t n, uint32_t lo, uint32_t cn, const uint64_t* rand, const uint8_t* sig_aff,
                                           const uint8_t* sig_use, const uint8_t* set_code, const uint8_t* sig_code, const uint8_t* msg_skip,
                                           uint8_t* msg_of_pos_out, uint8_t* negr_out, uint8_t* sigq_out, uint8_t* sskip_out) {
  if (n == 0 || m == 0 || cn == 0 || lo >= n || cn > n - lo) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem doff, dgs, dr, dsa, dsu, dsc, dgc, dms, comb, dmp, dnr, dsq, dsk;
  if (doff.put(grp_off, 4 * ((size_t)m + 1)) || dgs.put(grp_sets, 4 * (size_t)n) || dr.put(rand, 8 * (size_t)n) ||
      dsa.put(sig_aff, n * sizeof(tb::g2a)) || dsu.put(sig_use, n) || dsc.put(set_code, n) || dgc.put(sig_code, n) || dms.put(msg_skip, m))
    return -6;
  if (comb.out(TB_MSM_BUCKETS * sizeof(tb::g1a)) || dmp.out(4 * (size_t)n) || dnr.out(cn * sizeof(tb::g1a)) || dsq.out(cn * sizeof(tb::g2a)) ||
      dsk.out(cn))
    return -5;
  void* ac[] = {&comb.p};  // the device's (d 2^(8w)) g1 table, as dev_ctx builds it
  int rc = launch(dlsym(h, "k_g1_comb_init"), dim3(TB_MSM_BUCKETS / BLK), BLK, ac);
  void* a[] = {&doff.p, &dgs.p, &m, &n, &lo, &cn, &dr.p, &comb.p, &dsa.p, &dsu.p, &dsc.p, &dgc.p, &dms.p, &dmp.p, &dnr.p, &dsq.p, &dsk.p};
  if (!rc) rc = launch(dlsym(h, "k_gsettle_prep"), dim3(pad(cn) / BLK), BLK, a);
  if ((rc = finish(rc))) return rc;
  return dmp.get(msg_of_pos_out) || dnr.get(negr_out) || dsq.get(sigq_out) || dsk.get(sskip_out) ? -8 : 0;
}

extern "C" int tbls_test_pair_prod(const char* product_so, const uint8_t* in, uint32_t n, uint32_t chunk, uint32_t grid, uint8_t* out) {
  if (n == 0 || chunk == 0 || grid == 0 || (uint64_t)grid * chunk > 0xffffffffull) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem di, dout;
  if (di.put(in, n * F12)) return -6;
  if (dout.out(grid * F12)) return -5;
  void* a[] = {&di.p, &n, &chunk, &dout.p};
  if (const int rc = finish(launch(dlsym(h, "k_fp12_prod_wave"), dim3(grid), 64, a))) return rc;
  return dout.get(out) ? -8 : 0;
}

extern "C" int tbls_test_pair_prod_seg(const char* product_so, const uint8_t* in, uint32_t in_count, uint32_t n, uint32_t n_last,
                                       uint32_t nseg, uint32_t in_stride, uint32_t chunk, uint32_t grid_x, uint8_t* out, uint32_t out_stride) {
  if (nseg == 0 || nseg > 68 || chunk == 0 || grid_x == 0 || (uint64_t)grid_x * chunk > 0xffffffffull || grid_x > out_stride) return -1;
  // segment y reads in[y * in_stride .. + (y + 1 == nseg ? n_last : n))
  if ((uint64_t)(nseg - 1) * in_stride + n_last > in_count || (nseg > 1 && (uint64_t)(nseg - 2) * in_stride + n > in_count)) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem di, dout;
  if (di.put(in, in_count * F12)) return -6;
  if (dout.out(((size_t)(nseg - 1) * out_stride + grid_x) * F12)) return -5;
  void* a[] = {&di.p, &n, &n_last, &nseg, &in_stride, &chunk, &dout.p, &out_stride};
  if (const int rc = finish(launch(dlsym(h, "k_fp12_prod_wave_seg"), dim3(grid_x, nseg), 64, a))) return rc;
  return dout.get(out) ? -8 : 0;
}

extern "C" int tbls_test_pair_combine(const char* product_so, const uint8_t* vals, uint32_t nseg, uint8_t* out) {
  if (nseg == 0 || nseg > 68) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem dv, dout;
  if (dv.put(vals, nseg * F12)) return -6;
  if (dout.out(F12)) return -5;
  uint32_t dpack = 0;
  void* a[] = {&dv.p, &nseg, &dpack, &dout.p};
  if (const int rc = finish(launch(dlsym(h, "k_fp12_seg_combine_coop"), dim3(1), COOP, a))) return rc;
  return dout.get(out) ? -8 : 0;
}

extern "C" int tbls_test_pair_group_test(const char* product_so, const uint8_t* vals, uint32_t stride, uint32_t nseg, const uint32_t* list,
                                         uint32_t n_list, uint8_t* out) {
  if (stride == 0 || nseg == 0 || nseg > 68 || n_list == 0) return -1;
  for (uint32_t k = 0; k < n_list; k++)
    if (list[k] >= stride) return -1;  // segment j of group g at vals[j * stride + g]
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem dv, dl, dout;
  if (dv.put(vals, (size_t)nseg * stride * F12) || dl.put(list, 4 * (size_t)n_list)) return -6;
  if (dout.out(n_list)) return -5;
  void* a[] = {&dv.p, &stride, &nseg, &dl.p, &dout.p};
  if (const int rc = finish(launch(dlsym(h, "k_group_test_coop"), dim3(n_list), COOP, a))) return rc;
  return dout.get(out) ? -8 : 0;
}

extern "C" int tbls_test_pair_miller_wave(const char* product_so, const uint8_t* P, const uint8_t* Q, const uint8_t* skip,
                                          const uint8_t* code_a, const uint8_t* code_b, uint32_t n, uint8_t* f_out) {
  if (n == 0) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem dP, dQ, ds, da, db, df;
  if (dP.put(P, n * sizeof(tb::g1a)) || dQ.put(Q, n * sizeof(tb::g2a)) || ds.put(skip, n) || da.put(code_a, n) || db.put(code_b, n)) return -6;
  if (df.out(n * F12)) return -5;
  void* a[] = {&dP.p, &dQ.p, &ds.p, &da.p, &db.p, &n, &df.p};
  if (const int rc = finish(launch(dlsym(h, "k_miller_wave"), dim3(n), 64, a))) return rc;
  return df.get(f_out) ? -8 : 0;
}

// skip: the 2n bytes of a settle's pairs, read and returned (no guard: an in-place buffer)
extern "C" int tbls_test_pair_settle_mask(const char* product_so, const uint8_t* set_code, uint32_t n, uint8_t* skip /* 2n, in and out */) {
  if (n == 0) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem dc, ds;
  if (dc.put(set_code, n) || ds.put(skip, 2 * (size_t)n)) return -6;
  void* a[] = {&dc.p, &n, &ds.p};
  if (const int rc = finish(launch(dlsym(h, "k_settle_mask"), dim3((n + 255) / 256), 256, a))) return rc;
  return ds.get(skip) ? -8 : 0;
}
