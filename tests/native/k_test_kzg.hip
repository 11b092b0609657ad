// Direct launches of the KZG kernels in both of their forms.
// TEST INFRASTRUCTURE (libtekubls_test.so; never loaded by the product): it
// launches the PRODUCT library's own kernels -- looked up by name in the
// already-loaded libtekubls_hip.so, as k_test_hash.hip does -- on caller
// inputs, for tests/test_gpu_kzg_kernels.py to compare with the oracle.  The
// host API picks one form per batch size (tb_kzg.hip kzg_coop), so the suite's
// small batches never reach the one-lane forms through it.
//   stage 0  points: coop == 0 k_kzg_points, else k_kzg_points_coop
//            in  = n x 48 compressed bytes
//            out = n x 100: code (1), inf (1), 2 unused, x, y (48-byte
//                  big-endian plain integers; meaningful for code 0, inf 0)
//   stage 1  terms: coop == 0 k_kzg_terms, else k_kzg_terms_coop
//            in  = 2n affine points (commitments, then proofs; x || y as
//                  48-byte big-endian plain integers) || 2n infinity flags ||
//                  n z || n y || r (32-byte big-endian plain integers < r)
//            out = (3n + 1) x 100: u32 finite flag, affine x, y of T[k]
//                  (normalised here with the host build of jac_to_aff)
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../teku_amd/csrc/tb_glv.h"

namespace {
constexpr uint32_t BLK = 64;  // TB_BLOCK (tb_kdecl.h)
constexpr size_t REC = 100;

struct dev_mem {
  void* p = nullptr;
  ~dev_mem() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t n) { return hipMalloc(&p, n ? n : 1) == hipSuccess ? 0 : -1; }
};

int launch(void* fn, uint32_t grid, uint32_t block, void** args) {
  if (!fn) return -2;
  return hipLaunchKernel(fn, dim3(grid), dim3(block), args, 0, nullptr) == hipSuccess ? 0 : -3;
}

int up(const dev_mem& d, const void* h, size_t n) { return hipMemcpy(d.p, h, n, hipMemcpyHostToDevice) == hipSuccess ? 0 : -6; }
int down(void* h, const dev_mem& d, size_t n) { return hipMemcpy(h, d.p, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -8; }

int run_points(void* fn, int coop, const uint8_t* in, uint32_t m, uint8_t* out) {
  dev_mem db, dout, dinf, dcode;
  if (db.alloc(48 * (size_t)m) || dout.alloc(m * sizeof(tb::g1a)) || dinf.alloc(m) || dcode.alloc(m)) return -5;
  if (up(db, in, 48 * (size_t)m) || hipMemset(dout.p, 0, m * sizeof(tb::g1a)) != hipSuccess || hipMemset(dinf.p, 0xee, m) != hipSuccess ||
      hipMemset(dcode.p, 0xee, m) != hipSuccess)
    return -6;
  void* args[] = {&db.p, &m, &dout.p, &dinf.p, &dcode.p};
  if (int rc = coop ? launch(fn, (m + 3) / 4, 64, args) : launch(fn, (m + BLK - 1) / BLK, BLK, args)) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return -7;
  std::vector<tb::g1a> pts(m);
  std::vector<uint8_t> inf(m), code(m);
  if (down(pts.data(), dout, m * sizeof(tb::g1a)) || down(inf.data(), dinf, m) || down(code.data(), dcode, m)) return -8;
  for (uint32_t i = 0; i < m; i++) {
    uint8_t* o = out + REC * i;
    memset(o, 0, REC);
    o[0] = code[i];
    o[1] = inf[i];
    if (code[i] == 0 && inf[i] == 0) {
      tb::fp_plain_to_be(tb::fp_from_mont(pts[i].x), o + 4);
      tb::fp_plain_to_be(tb::fp_from_mont(pts[i].y), o + 52);
    }
  }
  return 0;
}

int run_terms(void* fn, int coop, const uint8_t* in, uint32_t n, uint8_t* out) {
  const uint32_t nt = 3 * n + 1;
  std::vector<tb::g1a> pts(2 * n);
  std::vector<tb::fr> zy(2 * n + 1);  // z, y, r
  const uint8_t* p_inf = in + 96 * (size_t)(2 * n);
  const uint8_t* p_sc = p_inf + 2 * n;
  for (uint32_t i = 0; i < 2 * n; i++) {
    pts[i].x = tb::fp_to_mont(tb::fp_plain_from_be(in + 96 * (size_t)i));
    pts[i].y = tb::fp_to_mont(tb::fp_plain_from_be(in + 96 * (size_t)i + 48));
  }
  for (uint32_t i = 0; i < 2 * n + 1; i++) zy[i] = tb::fr_to_mont(tb::fr_plain_from_be(p_sc + 32 * (size_t)i));
  dev_mem dp, dinf, dzy, dT;
  if (dp.alloc(pts.size() * sizeof(tb::g1a)) || dinf.alloc(2 * n) || dzy.alloc(zy.size() * sizeof(tb::fr)) || dT.alloc(nt * sizeof(tb::g1j)))
    return -5;
  if (up(dp, pts.data(), pts.size() * sizeof(tb::g1a)) || up(dinf, p_inf, 2 * n) || up(dzy, zy.data(), zy.size() * sizeof(tb::fr)) ||
      hipMemset(dT.p, 0xee, nt * sizeof(tb::g1j)) != hipSuccess)
    return -6;
  const tb::fr* z = static_cast<const tb::fr*>(dzy.p);
  const tb::fr *y = z + n, *r = z + 2 * n;
  uint32_t un = n;
  void* args[] = {&dp.p, &dinf.p, &z, &y, &r, &un, &dT.p};
  if (int rc = coop ? launch(fn, nt, 16, args) : launch(fn, (nt + BLK - 1) / BLK, BLK, args)) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return -7;
  std::vector<tb::g1j> T(nt);
  if (down(T.data(), dT, nt * sizeof(tb::g1j))) return -8;
  for (uint32_t k = 0; k < nt; k++) {
    uint8_t* o = out + REC * k;
    memset(o, 0, REC);
    tb::g1a a;
    if (tb::jac_to_aff(a, T[k])) {
      o[0] = 1;
      tb::fp_plain_to_be(tb::fp_from_mont(a.x), o + 4);
      tb::fp_plain_to_be(tb::fp_from_mont(a.y), o + 52);
    }
  }
  return 0;
}
}  // namespace

extern "C" int tbls_test_kzg_kernel(const char* product_so, int stage, int coop, const uint8_t* in, uint32_t n, uint8_t* out) {
  if (n == 0 || n > 4096) return -1;
  void* h = dlopen(product_so, RTLD_NOW | RTLD_NOLOAD);  // the instance the tests already use
  if (!h) h = dlopen(product_so, RTLD_NOW);
  if (!h) return -4;
  switch (stage) {
    case 0: return run_points(dlsym(h, coop ? "k_kzg_points_coop" : "k_kzg_points"), coop, in, n, out);
    case 1: return run_terms(dlsym(h, coop ? "k_kzg_terms_coop" : "k_kzg_terms"), coop, in, n, out);
    default: return -1;
  }
}
