// Byte-level parity hook of the key and signature stage kernels of a
// randomized batch, and of the hash kernel's randomizer branch.
// TEST INFRASTRUCTURE (libtekubls_test.so; never loaded by the product): like
// k_test_hash.hip it launches the PRODUCT library's own kernels -- looked up
// by name in the already-loaded libtekubls_hip.so -- with the grids and blocks
// of tb_lib.hip (launch_set_pk, key_chain, sig_chain) on caller inputs, and
// returns their raw outputs (Montgomery limbs, flags, codes, n_bad) for
// tests/test_gpu_stages.py to compare with tests/stage_cases.py.
//
// Every output buffer is preset to 0xEE (an unwritten slot shows); set_code,
// sig_code and n_bad are zeroed first, as the library does (the kernels write
// failures only); the comb table is built here with k_g1_comb_init.  Every HIP
// status is checked: the first failure returns a negative code and nothing
// more is launched.
//
// tbls_test_key_stage, variant:
//   0  k_pk_decompress + k_set_pk (multi 0)
//   1  k_pk_decompress + k_set_pk_w2 (multi 0)
//   2  k_keys_coop (grid (n + 3) / 4, block 128)
//   3  k_pk_decompress + k_set_pk (multi 1) + k_multi_list + k_set_pk_wave
//   4  k_pk_decompress + k_set_pk (multi 2) + k_multi_list + k_set_pk_agg_coop (block 512)
//   key_idx != null: the table form -- pks are the table's n_keys keys
//   (decompressed once), key_idx[pk_off[n]] addresses them, tab_n bounds them;
//   k_keys_coop then runs with pks null.
//   unit_r != 0 (variants 0, 1, 4): multi_wave | 4 / unit_r = 1, P = apk.
// tbls_test_sig_stage, variant:
//   0  k_sig_check (skip mode 1)   1  k_sig_check_w2 (skip mode 1)   2  k_sig_check_coop
//      -> q_out n * 192, flag_out n (skip flags), code_out n, n_bad
//   3  the bucket-sum chain of sig_chain with k_sig_check, 4 with k_sig_check_w2:
//      memset counts, k_msm_hist, k_msm_scan, k_msm_scatter, the check in skip
//      mode 0, k_msm_bucket_tree, k_msm_bitsum_pairs
//      -> p_out 64 * 96, q_out 64 * 192, flag_out 64 (skip), code_out n, n_bad,
//         total_out = off[2048], bucket_out (nullable) 2048 * 288: the bucket
//         sums (Jacobian; digit-0 slots stay 0xEE)
// tbls_test_hash_rand: k_set_hash_coop with rand non-null, Q = [r] H(m).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../teku_amd/csrc/tb_plan.h"

namespace {
constexpr uint32_t BLK = 64;  // TB_BLOCK (tb_kdecl.h)

struct dev_mem {
  void* p = nullptr;
  ~dev_mem() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t n) { return hipMalloc(&p, n ? n : 1) == hipSuccess ? 0 : -1; }
  // allocate and fill with one byte / with host data
  int fill(size_t n, int byte) { return alloc(n) || hipMemset(p, byte, n ? n : 1) != hipSuccess ? -1 : 0; }
  int put(const void* src, size_t n) { return alloc(n) || (n && hipMemcpy(p, src, n, hipMemcpyHostToDevice) != hipSuccess) ? -1 : 0; }
  int get(void* dst, size_t n) const { return hipMemcpy(dst, p, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
};

int launch(void* fn, uint32_t grid, uint32_t block, void** args) {
  if (!fn) return -2;
  return hipLaunchKernel(fn, dim3(grid), dim3(block), args, 0, nullptr) == hipSuccess ? 0 : -3;
}

void* product(const char* so) {
  void* h = dlopen(so, RTLD_NOW | RTLD_NOLOAD);  // the instance the tests already use
  return h ? h : dlopen(so, RTLD_NOW);
}

// the device's (d 2^(8w)) g1 table, as dev_ctx builds it
int make_comb(void* h, dev_mem& comb) {
  if (comb.fill(TB_MSM_BUCKETS * sizeof(tb::g1a), 0xee)) return -5;
  void* a[] = {&comb.p};
  return launch(dlsym(h, "k_g1_comb_init"), TB_MSM_BUCKETS / BLK, BLK, a);
}
}  // namespace

extern "C" int tbls_test_key_stage(const char* product_so, int variant, const uint8_t* pks, size_t n_keys, const uint32_t* pk_off,
                                   const uint32_t* key_idx, uint32_t tab_n, const uint64_t* rand, size_t n, int unit_r,
                                   uint8_t* p_out /* n * 96 */, uint8_t* p2_out /* n * 96 */, uint8_t* code_out /* n */,
                                   uint32_t* n_bad_out) {
  if (n == 0 || n_keys == 0 || variant < 0 || variant > 4) return -1;
  if (unit_r && (variant == 2 || variant == 3)) return -1;  // those kernels have no r = 1 form
  void* h = product(product_so);
  if (!h) return -4;
  auto sym = [&](const char* name) { return dlsym(h, name); };
  const size_t n_idx = pk_off[n];
  dev_mem dpks, doff, didx, drand, daff, dcode, dP, dP2, dset, dbad, dlist, dcnt, comb;
  if (dpks.put(pks, n_keys * 48) || doff.put(pk_off, 4 * (n + 1)) || (key_idx && didx.put(key_idx, 4 * n_idx)) || drand.put(rand, 8 * n)) return -6;
  if (daff.fill(n_keys * sizeof(tb::g1a), 0xee) || dcode.fill(n_keys, 0xee) || dP.fill(n * sizeof(tb::g1a), 0xee) ||
      dP2.fill(n * sizeof(tb::g1a), 0xee) || dset.fill(n, 0) || dbad.fill(4, 0) || dlist.fill(4 * n, 0xee) || dcnt.fill(4, 0))
    return -5;
  int rc = make_comb(h, comb);
  if (rc) return rc;
  uint32_t n32 = (uint32_t)n, k32 = (uint32_t)n_keys, tn = key_idx ? tab_n : 0u, unit = unit_r ? 1u : 0u;
  uint32_t multi = (variant == 3 ? 1u : variant == 4 ? 2u : 0u) | (unit_r ? 4u : 0u);
  const void* null = nullptr;
  const uint32_t g = (n32 + BLK - 1) / BLK;
  void* a_dec[] = {&dpks.p, &k32, &daff.p, &dcode.p};
  void* a_set[] = {&doff.p, &daff.p, &dcode.p, &drand.p, &n32, &dP.p, &dset.p, &dbad.p, &didx.p, &tn, &multi, &dP2.p, &comb.p};
  void* a_list[] = {&doff.p, &n32, &dlist.p, &dcnt.p};
  void* a_wave[] = {&doff.p, &daff.p, &dcode.p, &drand.p, &dlist.p, &dcnt.p, &dP.p, &dset.p, &dbad.p, &didx.p, &tn};
  void* a_agg[] = {&doff.p, &daff.p, &dcode.p, &drand.p, &dlist.p, &dcnt.p, &dP.p, &dset.p, &dbad.p, &didx.p, &tn, &dP2.p, &comb.p, &unit};
  // k_keys_coop: byte keys, or (pks null) the decompressed table
  void* a_coop_b[] = {&dpks.p, &doff.p, &null, &null, &null, &tn, &drand.p, &n32, &dP.p, &dP2.p, &dset.p, &dbad.p, &comb.p};
  void* a_coop_t[] = {&null, &doff.p, &daff.p, &dcode.p, &didx.p, &tn, &drand.p, &n32, &dP.p, &dP2.p, &dset.p, &dbad.p, &comb.p};
  if (variant != 2 || key_idx) rc = launch(sym("k_pk_decompress"), (k32 + BLK - 1) / BLK, BLK, a_dec);
  if (!rc) switch (variant) {
      case 0: rc = launch(sym("k_set_pk"), g, BLK, a_set); break;
      case 1: rc = launch(sym("k_set_pk_w2"), g, BLK, a_set); break;
      case 2: rc = launch(sym("k_keys_coop"), (n32 + 3) / 4, 128, key_idx ? a_coop_t : a_coop_b); break;
      default:  // launch_set_pk with multi
        rc = launch(sym("k_set_pk"), g, BLK, a_set);
        if (!rc) rc = launch(sym("k_multi_list"), g, BLK, a_list);
        if (!rc && variant == 3) rc = launch(sym("k_set_pk_wave"), std::min<uint32_t>(n32, 4096u), 64, a_wave);
        if (!rc && variant == 4) rc = launch(sym("k_set_pk_agg_coop"), std::min<uint32_t>(n32, 4096u), 512, a_agg);
    }
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return -7;
  if (dP.get(p_out, n * sizeof(tb::g1a)) || dP2.get(p2_out, n * sizeof(tb::g1a)) || dset.get(code_out, n) || dbad.get(n_bad_out, 4)) return -8;
  return 0;
}

extern "C" int tbls_test_sig_stage(const char* product_so, int variant, const uint8_t* sigs, const uint64_t* rand, size_t n,
                                   uint8_t* q_out, uint8_t* flag_out, uint8_t* code_out /* n */, uint32_t* n_bad_out,
                                   uint8_t* p_out /* chain: 64 * 96 */, uint32_t* total_out /* chain */,
                                   uint8_t* bucket_out /* chain, nullable: 2048 * 288 */) {
  if (n == 0 || variant < 0 || variant > 4) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  auto sym = [&](const char* name) { return dlsym(h, name); };
  const bool chain = variant >= 3;
  const size_t np = chain ? TB_MSM_XPAIRS : n;  // pairs returned
  dev_mem dsig, drand, daff, duse, dcode, dbad, dcnt, doffs, dcur, didx, dsum, dP, dQ, dskip, comb;
  if (dsig.put(sigs, n * 96) || (chain && drand.put(rand, 8 * n))) return -6;
  if (daff.fill(n * sizeof(tb::g2a), 0xee) || duse.fill(n, 0xee) || dcode.fill(n, 0) || dbad.fill(4, 0)) return -5;
  uint32_t n32 = (uint32_t)n, mode = chain ? 0u : 1u;
  const uint32_t g = (n32 + BLK - 1) / BLK;
  void* a_chk[] = {&dsig.p, &n32, &daff.p, &duse.p, &dcode.p, &dbad.p, &mode};
  int rc = 0;
  if (!chain) {
    rc = variant == 2 ? launch(sym("k_sig_check_coop"), (n32 + 3) / 4, 64, a_chk)  // the same list without the mode
                      : launch(sym(variant == 1 ? "k_sig_check_w2" : "k_sig_check"), g, BLK, a_chk);
  } else {
    if (dcnt.fill(TB_MSM_BUCKETS * 4, 0xee) || doffs.fill((TB_MSM_BUCKETS + 1) * 4, 0xee) || dcur.fill(TB_MSM_BUCKETS * 4, 0xee) ||
        didx.fill(n * 8 * 4, 0xee) || dsum.fill((size_t)TB_MSM_BUCKETS * sizeof(tb::g2j), 0xee) || dP.fill(np * sizeof(tb::g1a), 0xee) ||
        dQ.fill(np * sizeof(tb::g2a), 0xee) || dskip.fill(np, 0xee))
      return -5;
    rc = make_comb(h, comb);
    void* a_hist[] = {&drand.p, &n32, &dcnt.p};
    void* a_scan[] = {&dcnt.p, &doffs.p, &dcur.p};
    void* a_scat[] = {&drand.p, &n32, &dcur.p, &didx.p};
    void* a_tree[] = {&daff.p, &duse.p, &doffs.p, &didx.p, &dsum.p};
    void* a_bits[] = {&dsum.p, &comb.p, &dP.p, &dQ.p, &dskip.p};
    if (!rc && hipMemset(dcnt.p, 0, TB_MSM_BUCKETS * 4) != hipSuccess) rc = -6;
    if (!rc) rc = launch(sym("k_msm_hist"), g, BLK, a_hist);
    if (!rc) rc = launch(sym("k_msm_scan"), 1, 256, a_scan);
    if (!rc) rc = launch(sym("k_msm_scatter"), g, BLK, a_scat);
    if (!rc) rc = launch(sym(variant == 4 ? "k_sig_check_w2" : "k_sig_check"), g, BLK, a_chk);
    if (!rc) rc = launch(sym("k_msm_bucket_tree"), TB_MSM_TREE_WG, 64, a_tree);
    if (!rc) rc = launch(sym("k_msm_bitsum_pairs"), TB_MSM_XPAIRS, 64, a_bits);
  }
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return -7;
  if (dcode.get(code_out, n) || dbad.get(n_bad_out, 4)) return -8;
  if (!chain) return daff.get(q_out, n * sizeof(tb::g2a)) || duse.get(flag_out, n) ? -8 : 0;
  if (dP.get(p_out, np * sizeof(tb::g1a)) || dQ.get(q_out, np * sizeof(tb::g2a)) || dskip.get(flag_out, np) ||
      hipMemcpy(total_out, (const uint32_t*)doffs.p + TB_MSM_BUCKETS, 4, hipMemcpyDeviceToHost) != hipSuccess ||
      (bucket_out && dsum.get(bucket_out, (size_t)TB_MSM_BUCKETS * sizeof(tb::g2j))))
    return -8;
  return 0;
}

extern "C" int tbls_test_hash_rand(const char* product_so, const uint8_t* msgs, const uint32_t* msg_off, size_t n, const uint8_t* dst,
                                   size_t dlen, const uint64_t* rand, uint8_t* q_out /* n * 192 */, uint8_t* skip_out /* n */) {
  if (n == 0 || dlen > 255 || !rand) return -1;
  void* h = product(product_so);
  if (!h) return -4;
  dev_mem dm, doff, ddst, drand, dq, dskip;
  if (dm.put(msgs, msg_off[n]) || doff.put(msg_off, 4 * (n + 1)) || ddst.put(dst, dlen) || drand.put(rand, 8 * n)) return -6;
  if (dq.fill(n * sizeof(tb::g2a), 0xee) || dskip.fill(n, 0xee)) return -5;
  uint32_t n32 = (uint32_t)n, d32 = (uint32_t)dlen;
  void* a[] = {&dm.p, &doff.p, &ddst.p, &d32, &n32, &dq.p, &dskip.p, &drand.p};
  const int rc = launch(dlsym(h, "k_set_hash_coop"), n32, 256, a);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return -7;
  return dq.get(q_out, n * sizeof(tb::g2a)) || dskip.get(skip_out, n) ? -8 : 0;
}
