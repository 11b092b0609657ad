// Parity hook of the per-key comb kernels (teku_amd/csrc/tb_pkcomb.h,
// DESIGN.md 3n).  TEST INFRASTRUCTURE (libtekubls_test.so; never loaded by the
// product): like k_test_stages.hip it launches the PRODUCT library's own
// kernels -- looked up by name in the already-loaded libtekubls_hip.so -- with
// the grids and blocks of tb_lib.hip, on hand-made rows, and returns their raw
// outputs for tests/test_gpu_pkcomb.py.
//
// tbls_test_pkcomb, on n sets over n_keys byte keys (pk_off: n + 1 offsets):
//   1. k_pk_decompress of the keys;
//   2. a hand-made learned cache of n_keys rows (empty, fixed seed) and a miss
//      list naming every key: k_pk_learn_comb appends the valid keys and builds
//      the comb rows below comb_cap; k_pk_comb_build builds a table region with
//      a row per key;
//   3. k_pk_lookup_ref of the same keys against that cache -> ref_lookup_out;
//   4. the references the set kernel gets, per key by mode[j]: 0 none (not
//      ready), 1 what the lookup wrote (the cache's row), 2 the table region's
//      row j (none when the key is invalid) -> ref_used_out;
//   5. k_set_pk_comb_w2 with those references, k_set_pk_w2 on the same sets,
//      and with key_idx (nullable) k_set_pk_comb_w2 by index over the table
//      region (tab_n = n_keys);
//   6. stat_out: the comb counters (sets served -- both comb launches --, cache
//      rows built, table rows built).
// Every output buffer is preset to 0xEE; codes and n_bad are zeroed first, as
// the library does.  Every HIP status is checked: the first failure returns a
// negative code and nothing more is launched.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../teku_amd/csrc/tb_pkcomb.h"
#include "../../teku_amd/csrc/tb_pkindex.h"

namespace {
constexpr uint32_t BLK = 64;  // TB_BLOCK, TB_PKCOMB_BLOCK (tb_kdecl.h)

struct dev_mem {
  void* p = nullptr;
  ~dev_mem() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t n) { return hipMalloc(&p, n ? n : 1) == hipSuccess ? 0 : -1; }
  int fill(size_t n, int byte) { return alloc(n) || hipMemset(p, byte, n ? n : 1) != hipSuccess ? -1 : 0; }
  int put(const void* src, size_t n) { return alloc(n) || (n && hipMemcpy(p, src, n, hipMemcpyHostToDevice) != hipSuccess) ? -1 : 0; }
  int get(void* dst, size_t n) const { return hipMemcpy(dst, p, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
};

int launch(void* fn, uint32_t grid, uint32_t block, void** args) {
  if (!fn) return -2;
  return hipLaunchKernel(fn, dim3(grid), dim3(block), args, 0, nullptr) == hipSuccess ? 0 : -3;
}
}  // namespace

extern "C" int tbls_test_pkcomb(const char* product_so, const uint8_t* pks, size_t n_keys, const uint32_t* pk_off, const uint64_t* rand, size_t n,
                                const uint8_t* mode /* n_keys */, uint32_t comb_cap, const uint32_t* key_idx /* nullable: pk_off[n] */,
                                uint8_t* p_comb /* n * 96 */, uint8_t* code_comb /* n */, uint32_t* nbad_comb, uint8_t* p_w2, uint8_t* code_w2,
                                uint32_t* nbad_w2, uint8_t* p_idx /* with key_idx */, uint8_t* code_idx, uint32_t* nbad_idx,
                                uint32_t* ref_lookup_out /* n_keys */, uint32_t* ref_used_out /* n_keys */, uint64_t* stat_out /* 4 */) {
  if (n == 0 || n_keys == 0 || n_keys > 4096 || comb_cap > n_keys || pk_off[n] != n_keys) return -1;
  void* h = dlopen(product_so, RTLD_NOW | RTLD_NOLOAD);  // the instance the tests already use
  if (!h) h = dlopen(product_so, RTLD_NOW);
  if (!h) return -4;
  auto sym = [&](const char* name) { return dlsym(h, name); };
  const uint32_t K = (uint32_t)n_keys, slots = tb::pkx_capacity(K);
  uint32_t n32 = (uint32_t)n;
  std::vector<uint32_t> list(K + 1);
  list[0] = K;
  for (uint32_t j = 0; j < K; j++) list[1 + j] = j;

  dev_mem dpks, doff, drand, didx, daff, dcode, dslots, dkeys, dpoints, dhead, dlist, dready, dccomb, dtcomb, dstat;
  if (dpks.put(pks, n_keys * 48) || doff.put(pk_off, 4 * (n + 1)) || drand.put(rand, 8 * n) || (key_idx && didx.put(key_idx, 4 * n_keys)) ||
      dlist.put(list.data(), 4 * list.size()))
    return -6;
  if (daff.fill(n_keys * sizeof(tb::g1a), 0xee) || dcode.fill(n_keys, 0xee) || dslots.fill((size_t)slots * 4, 0) || dkeys.fill(n_keys * 48, 0xee) ||
      dpoints.fill(n_keys * 96, 0xee) || dhead.fill(64, 0) || dready.fill(comb_cap, 0) || dccomb.fill((size_t)comb_cap * TB_PKCOMB_ROW_BYTES, 0xee) ||
      dtcomb.fill(n_keys * TB_PKCOMB_ROW_BYTES, 0xee) || dstat.fill(32, 0))
    return -5;
  tb::pkx_cache cache = {(uint32_t*)dslots.p, slots - 1u, (uint32_t*)dkeys.p, (uint32_t*)dpoints.p, K, (uint32_t*)dhead.p,
                         (unsigned long long*)((uint8_t*)dhead.p + 8), 0x0123456789abcdefull};
  uint32_t k32 = K, align = 16, cap = comb_cap;
  const uint32_t bgrid = std::min<uint32_t>((K + BLK - 1) / BLK, 1024u);  // tb_lib.hip pkcomb_grid

  // 1, 2: the keys, the cache's rows and combs, the table region
  void* a_dec[] = {&dpks.p, &k32, &daff.p, &dcode.p};
  void* a_learn[] = {&dpks.p, &align, &dlist.p, &daff.p, &dcode.p, &cache, &dccomb.p, &dready.p, &cap, &dstat.p};
  void* a_build[] = {&daff.p, &dcode.p, &k32, &dtcomb.p, &dstat.p};
  int rc = launch(sym("k_pk_decompress"), (K + BLK - 1) / BLK, BLK, a_dec);
  if (!rc) rc = launch(sym("k_pk_learn_comb"), bgrid, BLK, a_learn);
  if (!rc) rc = launch(sym("k_pk_comb_build"), bgrid, BLK, a_build);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return -7;

  // 3: the lookup's references
  dev_mem daff2, dcode2, dmiss, dlstat, dref, dused;
  if (daff2.fill(n_keys * sizeof(tb::g1a), 0xee) || dcode2.fill(n_keys, 0xee) || dmiss.fill(4 * (n_keys + 1), 0) || dlstat.fill(16, 0) ||
      dref.fill(4 * n_keys, 0xee))
    return -5;
  const void* null = nullptr;
  uint32_t zero = 0;
  uint64_t seed0 = 0;
  void* a_look[] = {&dpks.p, &k32, &align, &null, &zero, &seed0, &null, &null, &null, &cache, &daff2.p, &dcode2.p, &dmiss.p, &dlstat.p,
                    &dref.p, &dready.p, &cap, &zero};
  rc = launch(sym("k_pk_lookup_ref"), (K + 255) / 256, 256, a_look);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return -7;
  std::vector<uint32_t> ref(K), used(K);
  std::vector<uint8_t> code(K);
  if (dref.get(ref.data(), 4 * n_keys) || dcode.get(code.data(), n_keys)) return -8;
  for (uint32_t j = 0; j < K; j++) {
    ref_lookup_out[j] = ref[j];
    used[j] = mode[j] == 1 ? ref[j] : mode[j] == 2 ? tb::comb_ref(true, j, code[j] == TB_SUCCESS) : TB_PKREF_NONE;
    if ((used[j] & TB_PKREF_READY) && !(used[j] & TB_PKREF_TABLE) && (used[j] & TB_PKREF_ROW) >= comb_cap) return -9;  // a row the region lacks
    ref_used_out[j] = used[j];
  }
  if (dused.put(used.data(), 4 * n_keys)) return -6;

  // 5: the set kernels
  const uint32_t g = (n32 + BLK - 1) / BLK;
  uint32_t tab0 = 0, tabn = K, multi = 0;
  struct out_set {
    dev_mem P, code, bad;
    int init(size_t n) { return P.fill(n * sizeof(tb::g1a), 0xee) || code.fill(n, 0) || bad.fill(4, 0) ? -5 : 0; }
    int fetch(size_t n, uint8_t* p, uint8_t* c, uint32_t* b) const { return P.get(p, n * sizeof(tb::g1a)) || code.get(c, n) || bad.get(b, 4) ? -8 : 0; }
  } oc, ow, oi;
  if (oc.init(n) || ow.init(n) || (key_idx && oi.init(n))) return -5;
  void* a_comb[] = {&doff.p, &daff.p, &dcode.p, &drand.p, &n32, &oc.P.p, &oc.code.p, &oc.bad.p, &null, &tab0, &multi, &null, &null,
                    &dused.p, &dccomb.p, &dtcomb.p, &dstat.p};
  void* a_w2[] = {&doff.p, &daff.p, &dcode.p, &drand.p, &n32, &ow.P.p, &ow.code.p, &ow.bad.p, &null, &tab0, &multi, &null, &null};
  void* a_idx[] = {&doff.p, &daff.p, &dcode.p, &drand.p, &n32, &oi.P.p, &oi.code.p, &oi.bad.p, &didx.p, &tabn, &multi, &null, &null,
                   &null, &null, &dtcomb.p, &dstat.p};
  rc = launch(sym("k_set_pk_comb_w2"), g, BLK, a_comb);
  if (!rc) rc = launch(sym("k_set_pk_w2"), g, BLK, a_w2);
  if (!rc && key_idx) rc = launch(sym("k_set_pk_comb_w2"), g, BLK, a_idx);
  if (rc) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return -7;
  if (oc.fetch(n, p_comb, code_comb, nbad_comb) || ow.fetch(n, p_w2, code_w2, nbad_w2) || (key_idx && oi.fetch(n, p_idx, code_idx, nbad_idx)))
    return -8;
  return dstat.get(stat_out, 32) ? -8 : 0;
}
