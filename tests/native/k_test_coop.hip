// Test library libtekubls_test.so, second translation unit (tests only): the
// lane-cooperative arithmetic (teku_amd/csrc/tb_coop.h, tb_cfe.h) test hooks,
// dispatched by tbls_test_ops in k_test.hip.
#include "../../teku_amd/csrc/tb_kdecl.h"
#include "tb_testops.h"
#include "../../teku_amd/csrc/tb_cfe.h"
#include "../../teku_amd/csrc/tb_cinv.h"
#include "tb_cpoint_ops.h"

using namespace tb;

// ---- lane-cooperative products (tb_coop.h) ----
// the row's digits -> [0, 2p) on lane 0 of the row (through LDS)
__device__ fp coop_row_to_fp(coop::c32 d, int32_t (*lds)[16]) {
  const int row = threadIdx.x >> 4;
  lds[row][threadIdx.x & 15] = d;
  __syncthreads();
  fp r = fp_zero();
  if ((threadIdx.x & 15) == 0) r = coop::cdigits_to_fp(lds[row]);
  __syncthreads();
  return r;
}

// 12 words of a [0, 2p) value, staged by the row's lane 0, -> the row's digits
__device__ coop::c32 coop_row_from_fp(const fp& v, uint32_t (*lds)[12]) {
  const int row = threadIdx.x >> 4;
  if ((threadIdx.x & 15) == 0)
    for (int i = 0; i < 12; i++) lds[row][i] = v.l[i];
  __syncthreads();
  const coop::c32 d = coop::cfrom_words(lds[row]);
  __syncthreads();
  return d;
}

// one product per 16-lane row: record = a (48 B) | b (48 B), out = a b (48 B)
extern "C" __global__ void __launch_bounds__(64) k_test_coop_mul(const uint8_t* in, uint8_t* out, uint32_t n) {
  __shared__ uint32_t W[4][12];
  __shared__ int32_t D[4][16];
  const coop::cctx K = coop::cctx_load();
  const uint32_t rec = blockIdx.x * 4 + (threadIdx.x >> 4);
  const bool live = rec < n;
  const uint8_t* r = in + (size_t)(live ? rec : 0) * TB_TEST_IN;
  fp a = fp_zero(), b = fp_zero();
  if ((threadIdx.x & 15) == 0) {
    a = tio_fp(r);
    b = tio_fp(r + 48);
  }
  const coop::c32 x = coop_row_from_fp(a, W), y = coop_row_from_fp(b, W);
  const fp z = coop_row_to_fp(coop::cmul(x, y, K), D);
  if (live && (threadIdx.x & 15) == 0) tio_put_fp(out + (size_t)rec * TB_TEST_OUT, z);
}

// timing: clock64 cycles of 64 chained coop products (one chain per row), of
// 64 steps of two interleaved chains, and of 64 chained lone-lane fp_mul;
// out = 3 x u64 (+0, +8, +16), then x = a b^64 (+64) and y = b a^64 (+112)
extern "C" __global__ void __launch_bounds__(64) k_test_coop_timing(const uint8_t* in, uint8_t* out) {
  __shared__ uint32_t W[4][12];
  __shared__ int32_t D[4][16];
  fp a = fp_zero(), b = fp_zero();
  if ((threadIdx.x & 15) == 0) {
    a = tio_fp(in);
    b = tio_fp(in + 48);
  }
  const coop::cctx K = coop::cctx_load();
  coop::c32 x = coop_row_from_fp(a, W), y = coop_row_from_fp(b, W);
  const coop::c32 x0 = x, y0 = y;
  const long long t0 = clock64();
  TB_NOUNROLL for (int k = 0; k < 64; k++) x = coop::cmul(x, y0, K);
  __syncthreads();
  const long long t1 = clock64();
  coop::c32 u = x0, v = y0;
  TB_NOUNROLL for (int k = 0; k < 64; k++) {
    u = coop::cmul(u, y0, K);
    v = coop::cmul(v, x0, K);
  }
  __syncthreads();
  const long long t2 = clock64();
  fp c = a;
  if (threadIdx.x == 0)
    for (int k = 0; k < 64; k++) c = fp_mul(c, b);
  __syncthreads();
  const long long t3 = clock64();
  const fp fx = coop_row_to_fp(x, D), fv = coop_row_to_fp(v, D);
  if (threadIdx.x == 0) {
    uint64_t* o = reinterpret_cast<uint64_t*>(out);
    o[0] = (uint64_t)(t1 - t0);
    o[1] = (uint64_t)(t2 - t1);
    o[2] = (uint64_t)(t3 - t2);
    tio_put_fp(out + 64, fx);
    tio_put_fp(out + 112, fv);
    tio_put_fp(out + 160, c);
  }
}

// test hook: the lane-cooperative final exponentiation (tb_cfe.h), one
// 256-thread block per record (tb_testops.h Fp12 layout); also the block's
// clock64 cycles at +576 (u64, little-endian)
extern "C" __global__ void __launch_bounds__(CFE_THREADS) k_test_final_exp_coop(const uint8_t* in, uint8_t* out) {
  __shared__ cfe_lds L;
  cfe::init(L);
  cfe_regs R;
  cfe::regs_load(R, L);
  const coop::cctx& K = R.K;
  if (threadIdx.x == 0) fp12_to_coords(L.tmp, tio_fp12(in + (size_t)blockIdx.x * TB_TEST_IN));
  __syncthreads();
  cfe::load_coords(L.F, L.tmp);
  const long long t0 = clock64();
  cfe::final_exp(L, R);
  const long long t1 = clock64();
  cfe::store_coords(L.F, L);
  if (threadIdx.x == 0) {
    uint8_t* o = out + (size_t)blockIdx.x * TB_TEST_OUT;
    tio_put_fp12(o, fp12_from_coords(L.tmp));
    *reinterpret_cast<uint64_t*>(o + 576) = (uint64_t)(t1 - t0);
  }
}


// test hook: single coop Fp12 ops (tb_cfe.h), one 256-thread block per record:
// in = x (Fp12, +0) | y (Fp12, +576) | op (u32 at +1152): 0 mul, 1 cyc_sqr,
// 2 frob, 3 conj, 4 load/store round trip; out = result (Fp12)
extern "C" __global__ void __launch_bounds__(256) k_test_cfe_ops(const uint8_t* in, uint8_t* out) {
  __shared__ cfe_lds L;
  const uint8_t* r = in + (size_t)blockIdx.x * TB_TEST_IN;
  cfe::init(L);
  cfe_regs R;
  cfe::regs_load(R, L);
  const coop::cctx& K = R.K;
  const uint32_t op = *reinterpret_cast<const uint32_t*>(r + 1152);
  if (threadIdx.x == 0) fp12_to_coords(L.tmp, tio_fp12(r));
  __syncthreads();
  cfe::load_coords(L.F, L.tmp);
  if (threadIdx.x == 0) fp12_to_coords(L.tmp, tio_fp12(r + 576));
  __syncthreads();
  cfe::load_coords(L.X, L.tmp);
  if (op == 0) cfe::mul(L.T, L.F, L.X, L, R);
  else if (op == 1) cfe::cyc_sqr(L.T, L.F, L, R);
  else if (op == 2) cfe::frob(L.T, L.F, L, R);
  else if (op == 3) cfe::conj(L.T, L.F);
  else if (op == 5) {  // the coop Fp12 inversion
    cfe::inv(L.T, L.F, L, R);
  } else if (op == 6) {  // t^x
    cfe::cyc_exp_x(L.T, L.F, L, R);
  } else if (op == 7) {  // full
    cfe::final_exp(L, R);
    cfe::copy(L.T, L.F);
  } else
    cfe::copy(L.T, L.F);
  // timing (clock64 of 64 levels of each kind, then one inversion; +576, +584, +592)
  long long c[4] = {0, 0, 0, 0};
  if (op == 8) {
    c[0] = clock64();
    for (int k = 0; k < 64; k++) cfe::cyc_sqr(L.A, L.A, L, R);
    c[1] = clock64();
    for (int k = 0; k < 64; k++) cfe::mul(L.B, L.B, L.F, L, R);
    c[2] = clock64();
    cfe::inv(L.C, L.F, L, R);
    c[3] = clock64();
  }
  cfe::store_coords(L.T, L);
  if (threadIdx.x == 0) {
    uint8_t* o = out + (size_t)blockIdx.x * TB_TEST_OUT;
    tio_put_fp12(o, fp12_from_coords(L.tmp));
    uint64_t* t = reinterpret_cast<uint64_t*>(o + 576);
    t[0] = (uint64_t)(c[1] - c[0]);
    t[1] = (uint64_t)(c[2] - c[1]);
    t[2] = (uint64_t)(c[3] - c[2]);
  }
}

// the row inversion (tb_cinv.h): one inversion per 16-lane row, record = a
// (48 B), out = a^-1 (48 B) at +0; record 0's row also times one row
// inversion and one lone-lane fp_inv (clock64 cycles, u64 at +48 / +56)
extern "C" __global__ void __launch_bounds__(64) k_test_coop_inv(const uint8_t* in, uint8_t* out, uint32_t n) {
  __shared__ int32_t D[4][16];
  const uint32_t row = threadIdx.x >> 4, rec = blockIdx.x * 4 + row;
  const bool live = rec < n;
  const fp a = tio_fp(in + (size_t)(live ? rec : 0) * TB_TEST_IN);  // every lane decodes the same record
  const long long t0 = clock64();
  const fp z = cinv::inv_row_lane0(a, D[row]);
  const long long t1 = clock64();
  fp y = a;
  if (rec == 0 && (threadIdx.x & 15) == 0) y = fp_inv(a);
  const long long t2 = clock64();
  if (live && (threadIdx.x & 15) == 0) {
    tio_put_fp(out + (size_t)rec * TB_TEST_OUT, z);
    if (rec == 0) {
      uint64_t* o = reinterpret_cast<uint64_t*>(out + 48);
      o[0] = (uint64_t)(t1 - t0);
      o[1] = (uint64_t)(t2 - t1);
      tio_put_fp(out + 64, y);
    }
  }
}

// ---- the row arithmetic at its edges (tests/coop_cases.py, tests/test_gpu_coop.py) ----
// Raw digits and raw limbs in and out, so the operands are not limited to what
// tio_fp produces (canonical values, class-1 digits).

// cmul on digit vectors: record = 16 int32 digits of a | 16 of b (little-endian,
// digit j for lane j), out = the 16 digits of cmul(a, b); four rows per wave,
// each with its own record (tbls_hostsim_coop_mul_digits on the GPU)
extern "C" __global__ void __launch_bounds__(64) k_test_coop_mul_digits(const uint8_t* in, uint8_t* out, uint32_t n) {
  const coop::cctx K = coop::cctx_load();
  const uint32_t rec = blockIdx.x * 4 + (threadIdx.x >> 4), j = threadIdx.x & 15;
  const bool live = rec < n;
  const int32_t* r = reinterpret_cast<const int32_t*>(in + (size_t)(live ? rec : 0) * TB_TEST_IN);
  const coop::c32 z = coop::cmul(r[j], r[16 + j], K);
  if (live) reinterpret_cast<int32_t*>(out + (size_t)rec * TB_TEST_OUT)[j] = z;
}

// cfrom_words -> cmul -> cdigits_to_fp on raw 12-word operands: record = a | b
// (48-byte big-endian plain integers below 2^384, no Montgomery conversion),
// out = the raw [0, 2p) result (tbls_hostsim_coop_mul_fp on the GPU)
extern "C" __global__ void __launch_bounds__(64) k_test_coop_mul_words(const uint8_t* in, uint8_t* out, uint32_t n) {
  __shared__ uint32_t W[4][12];
  __shared__ int32_t D[4][16];
  const coop::cctx K = coop::cctx_load();
  const uint32_t rec = blockIdx.x * 4 + (threadIdx.x >> 4);
  const bool live = rec < n;
  const uint8_t* r = in + (size_t)(live ? rec : 0) * TB_TEST_IN;
  fp a = fp_zero(), b = fp_zero();
  if ((threadIdx.x & 15) == 0) {
    a = fp_plain_from_be(r);
    b = fp_plain_from_be(r + 48);
  }
  const coop::c32 x = coop_row_from_fp(a, W), y = coop_row_from_fp(b, W);
  const fp z = coop_row_to_fp(coop::cmul(x, y, K), D);
  if (live && (threadIdx.x & 15) == 0) fp_plain_to_be(z, out + (size_t)rec * TB_TEST_OUT);
}

// cdigits_to_fp, one lane per record: record = 16 int32 signed digits, out =
// the raw [0, 2p) value (48-byte big-endian)
extern "C" __global__ void __launch_bounds__(64) k_test_coop_to_fp(const uint8_t* in, uint8_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const fp z = coop::cdigits_to_fp(reinterpret_cast<const int32_t*>(in + (size_t)i * TB_TEST_IN));
  fp_plain_to_be(z, out + (size_t)i * TB_TEST_OUT);
}

// creduce64 (the device branch): record = 16 int64 digit sums, out = 16 int32
// digits; four rows per wave
extern "C" __global__ void __launch_bounds__(64) k_test_coop_reduce(const uint8_t* in, uint8_t* out, uint32_t n) {
  const coop::cctx K = coop::cctx_load();
  const uint32_t rec = blockIdx.x * 4 + (threadIdx.x >> 4), j = threadIdx.x & 15;
  const bool live = rec < n;
  const int64_t* r = reinterpret_cast<const int64_t*>(in + (size_t)(live ? rec : 0) * TB_TEST_IN);
  const coop::c32 z = coop::creduce64(r[j], K.plo[0]);
  if (live) reinterpret_cast<int32_t*>(out + (size_t)rec * TB_TEST_OUT)[j] = z;
}

// inv_row_lane0<false> on raw limbs: record = a (48-byte big-endian, in [0, 2p),
// not p; no Montgomery conversion), out = the raw result; four rows per wave
extern "C" __global__ void __launch_bounds__(64) k_test_coop_inv_raw(const uint8_t* in, uint8_t* out, uint32_t n) {
  __shared__ int32_t D[4][16];
  const uint32_t row = threadIdx.x >> 4, rec = blockIdx.x * 4 + row;
  const bool live = rec < n;
  const fp a = fp_plain_from_be(in + (size_t)(live ? rec : 0) * TB_TEST_IN);  // every lane decodes the same record
  const fp z = cinv::inv_row_lane0<false>(a, D[row]);
  if (live && (threadIdx.x & 15) == 0) fp_plain_to_be(z, out + (size_t)rec * TB_TEST_OUT);
}

// inv_row_lane0<true> (scalar divsteps, early exit) the way the product calls
// it: one 64-lane block per record, only row (rec & 3) active behind a branch.
// out = the raw result, then the call's clock64 cycles (u64 at +48)
extern "C" __global__ void __launch_bounds__(64) k_test_coop_inv_u(const uint8_t* in, uint8_t* out) {
  __shared__ int32_t D[16];
  const uint32_t rec = blockIdx.x, row = threadIdx.x >> 4;
  const fp a = fp_plain_from_be(in + (size_t)rec * TB_TEST_IN);
  if (row == (rec & 3u)) {
    const long long t0 = clock64();
    const fp z = cinv::inv_row_lane0<true>(a, D);
    const long long t1 = clock64();
    if ((threadIdx.x & 15) == 0) {
      uint8_t* o = out + (size_t)rec * TB_TEST_OUT;
      fp_plain_to_be(z, o);
      *reinterpret_cast<uint64_t*>(o + 48) = (uint64_t)(t1 - t0);
    }
  }
}

// row point arithmetic (tb_cpoint.h), the ops of tb_cpoint_ops.h: one record
// per row, four rows per wave.  record = x1, y1, x2, y2 (tio_fp / tio_fp2
// coordinates; G2 fills 384 bytes, G1 the first 192), op (u32 at +384), the
// scalar (u64 at +392); out = X, Y, Z through cdigits_to_fp as raw 48-byte
// values (Montgomery form)
__device__ uint64_t tio_u64(const uint8_t* b) { return (uint64_t)tio_u32(b) | ((uint64_t)tio_u32(b + 4) << 32); }

template <int N>
__device__ void cpoint_load(coop::c32 (&v)[N], const uint8_t* r, uint32_t (*W)[12]) {
  TB_NOUNROLL for (int i = 0; i < N; i++) {
    fp a = fp_zero();
    if ((threadIdx.x & 15) == 0) a = tio_fp(r + 48 * i);
    v[i] = coop_row_from_fp(a, W);
  }
}

template <int N>
__device__ void cpoint_store(const coop::c32 (&v)[N], uint8_t* o, bool live, int32_t (*D)[16]) {
  TB_UNROLL for (int i = 0; i < N; i++) {
    const fp z = coop_row_to_fp(v[i], D);
    if (live && (threadIdx.x & 15) == 0) fp_plain_to_be(z, o + 48 * i);
  }
}

extern "C" __global__ void __launch_bounds__(64) k_test_cpoint_g1(const uint8_t* in, uint8_t* out, uint32_t n) {
  __shared__ uint32_t W[4][12];
  __shared__ int32_t D[4][16];
  const coop::cctx K = coop::cctx_load();
  const uint32_t rec = blockIdx.x * 4 + (threadIdx.x >> 4);
  const bool live = rec < n;
  const uint8_t* r = in + (size_t)(live ? rec : 0) * TB_TEST_IN;
  coop::c32 v[4];
  cpoint_load<4>(v, r, W);
  const coop::c32 one = coop::cfrom_words(R1);
  const coop::cj1 p = coop::cpoint_op<coop::cj1, coop::c32>((int)tio_u32(r + 384), v[0], v[1], v[2], v[3], one, tio_u64(r + 392), K);
  const coop::c32 c[3] = {p.x, p.y, p.z};
  cpoint_store<3>(c, out + (size_t)(live ? rec : 0) * TB_TEST_OUT, live, D);
}

extern "C" __global__ void __launch_bounds__(64) k_test_cpoint_g2(const uint8_t* in, uint8_t* out, uint32_t n) {
  __shared__ uint32_t W[4][12];
  __shared__ int32_t D[4][16];
  const coop::cctx K = coop::cctx_load();
  const uint32_t rec = blockIdx.x * 4 + (threadIdx.x >> 4);
  const bool live = rec < n;
  const uint8_t* r = in + (size_t)(live ? rec : 0) * TB_TEST_IN;
  coop::c32 v[8];
  cpoint_load<8>(v, r, W);
  const coop::c2 one = {coop::cfrom_words(R1), coop::c32(0)};
  const coop::cj2 p = coop::cpoint_op<coop::cj2, coop::c2>((int)tio_u32(r + 384), {v[0], v[1]}, {v[2], v[3]}, {v[4], v[5]}, {v[6], v[7]}, one,
                                                          tio_u64(r + 392), K);
  const coop::c32 c[6] = {p.x.c0, p.x.c1, p.y.c0, p.y.c1, p.z.c0, p.z.c1};
  cpoint_store<6>(c, out + (size_t)(live ? rec : 0) * TB_TEST_OUT, live, D);
}
