// CPU check of the per-key fixed-base comb (teku_amd/csrc/tb_pkcomb.h:
// comb_build, comb_mul_u64, the reference word and the ready bytes;
// tests/test_pkcomb_check.py) -- the functions k_pk_learn_comb, k_pk_comb_build
// and k_set_pk_comb_w2 run on the device.  Built with AddressSanitizer +
// UndefinedBehaviorSanitizer and run directly.  The arguments are compressed
// public keys in hex (the wrapper passes interop keys); without any, small
// multiples of the generator stand in.  Every row and every working array has
// its exact size, so an index past either is a sanitizer report.  Prints
// "failures 0" when every case holds.
//
// "count" as the first argument (a build with -DTB_COUNT_MULS,
// tools/count_muls.py): prints the Fp products of one comb_mul_u64 + jac_to_aff
// and of one comb_build instead.
#include <cstdio>
#include <cstring>
#include <vector>

#if defined(TB_COUNT_MULS)
extern "C" {
unsigned long long tb_mul_count = 0;
unsigned long long tb_sqr_count = 0;
unsigned long long tb_fp2mul_count = 0;
}
#endif
#include "tb_codec.h"
#include "tb_pkcomb.h"

using namespace tb;

static int failures = 0;
#define CHECK(c)                                         \
  do {                                                   \
    if (!(c)) {                                          \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      failures++;                                        \
    }                                                    \
  } while (0)

static bool same_fp(const fp& a, const fp& b) {
  const fp x = fp_canon(a), y = fp_canon(b);
  return memcmp(&x, &y, sizeof x) == 0;
}
// both to affine, canonical form, exact
static bool same_point(const g1j& a, const g1j& b) {
  g1a p, q;
  if (!jac_to_aff(p, a) || !jac_to_aff(q, b)) return false;
  return same_fp(p.x, q.x) && same_fp(p.y, q.y);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {  // splitmix64, seeded
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// the scalar whose comb digit is d in column j and zero elsewhere
static uint64_t column(uint32_t d, int j) {
  uint64_t r = 0;
  for (int t = 0; t < 4; t++)
    if (d >> t & 1) r |= 1ull << (16 * t + j);
  return r;
}

static std::vector<uint64_t> scalars() {
  std::vector<uint64_t> v = {1, 2, 1ull << 15, 1ull << 16, (1ull << 16) + 1, 1ull << 48, 1ull << 63, ~0ull};
  v.push_back(0xbeefull);                // the top three teeth all zero
  v.push_back(0x7ffe7ffe7ffe7ffeull);    // zero digits in columns 15 and 0
  v.push_back(0x7ffe00007ffe0000ull | 0x0000123400000000ull);
  for (uint32_t d = 1; d <= 15; d++) v.push_back(column(d, (int)(d % 16)) | (rng() & (((1ull << (d % 16)) - 1) * 0x0001000100010001ull)));  // entry d starts the walk
  v.push_back(column(15, 0));            // the sixteenth: the walk is column 0 alone
  for (int i = 0; i < 300; i++) v.push_back(rng() | 1ull << (rng() & 63));
  return v;
}

static std::vector<g1a> keys_from(int argc, char** argv) {
  std::vector<g1a> keys;
  for (int a = 1; a < argc; a++) {
    uint8_t b[48];
    if (strlen(argv[a]) != 96) continue;
    for (int i = 0; i < 48; i++) {
      unsigned v = 0;
      sscanf(argv[a] + 2 * i, "%2x", &v);
      b[i] = (uint8_t)v;
    }
    g1a p;
    bool inf = false;
    CHECK(g1_decompress(p, inf, b) == TB_SUCCESS && !inf);
    keys.push_back(p);
  }
  if (keys.empty()) {
    const g1j g = {fp_from_const(G1_X), fp_from_const(G1_Y), fp_one()};
    for (uint64_t k : {1ull, 3ull, 0x123456789abcdefull}) {
      g1a p;
      CHECK(jac_to_aff(p, jac_mul_u64(g, k)));
      keys.push_back(p);
    }
  }
  return keys;
}

int main(int argc, char** argv) {
  const bool count = argc > 1 && !strcmp(argv[1], "count");
  const std::vector<g1a> keys = keys_from(count ? 1 : argc, argv);
  std::vector<g1a> row(TB_PKCOMB_ENTRIES);
  std::vector<fp> tmp(TB_PKCOMB_TMP);

#if defined(TB_COUNT_MULS)
  if (count) {
    ::tb_mul_count = ::tb_sqr_count = 0;  // the stand-in keys' own products
    comb_build(row.data(), keys[0], tmp.data(), 1);
    const unsigned long long build = ::tb_mul_count, build_sq = ::tb_sqr_count;
    const uint64_t r = 0xF123456789ABCDEFull;  // tools/count_muls.py's randomizer: every column has a digit
    ::tb_mul_count = ::tb_sqr_count = 0;
    g1a out;
    (void)jac_to_aff(out, comb_mul_u64(row.data(), r));
    printf("set_pk_comb %llu %llu\npk_comb_build %llu %llu\n", ::tb_mul_count, ::tb_sqr_count, build, build_sq);
    return 0;
  }
#endif

  const std::vector<uint64_t> rs = scalars();
  for (const g1a& pk : keys) {
    for (g1a& e : row) memset(&e, 0xee, sizeof e);
    comb_build(row.data(), pk, tmp.data(), 1);
    // each entry against [d_comb] pk, d_comb = sum over the bits t of d of 2^(16 t)
    for (uint32_t d = 1; d <= TB_PKCOMB_ENTRIES; d++) CHECK(same_point(jac_from_aff(row[d - 1]), jac_mul_u64(jac_from_aff(pk), column(d, 0))));
    // a strided working array (the device's LDS columns) gives the same row
    {
      std::vector<g1a> row2(TB_PKCOMB_ENTRIES);
      std::vector<fp> tmp2((TB_PKCOMB_TMP - 1) * 5 + 1);
      comb_build(row2.data(), pk, tmp2.data(), 5);
      CHECK(memcmp(row.data(), row2.data(), TB_PKCOMB_ROW_BYTES) == 0);
    }
    for (uint64_t r : rs) {
      const bool ok = same_point(comb_mul_u64(row.data(), r), g1_mul_u64_aff_w2(pk, r));
      if (!ok) printf("FAIL r = %016llx\n", (unsigned long long)r);
      CHECK(ok);
    }
  }

  // the scalar list covers what it says: every entry starts a walk, zero top teeth, zero digits at both ends
  {
    bool first[16] = {false};
    for (uint64_t r : rs) {
      int j = 15;
      while (comb_digit(r, j) == 0) j--;
      first[comb_digit(r, j)] = true;
    }
    for (uint32_t d = 1; d <= 15; d++) CHECK(first[d]);
    CHECK(comb_digit(0xbeefull, 15) == 1 && comb_digit(0xbeefull, 4) == 0 && (0xbeefull >> 16) == 0);
    CHECK(comb_digit(0x7ffe7ffe7ffe7ffeull, 15) == 0 && comb_digit(0x7ffe7ffe7ffe7ffeull, 0) == 0 && comb_digit(0x7ffe7ffe7ffe7ffeull, 7) == 15);
    for (uint32_t d = 0; d <= 15; d++)
      for (int j = 0; j < 16; j++) CHECK(comb_digit(column(d, j), j) == d);
  }

  // ready bytes and the cap: a row at or beyond the cap never becomes ready,
  // and the reference word carries source, row and readiness
  {
    const uint32_t ROWS = 8, CAP = 5;
    std::vector<uint8_t> ready(CAP, 0);  // exactly the cap: marking a row beyond it would be out of bounds
    for (uint32_t r = 0; r < ROWS; r++) comb_mark_ready(ready.data(), r, CAP);
    for (uint32_t r = 0; r < ROWS; r++) {
      const bool is_ready = comb_row_in_cap(r, CAP) && ready[r];
      CHECK(is_ready == (r < CAP));
      const uint32_t ref = comb_ref(false, r, is_ready);
      CHECK(r < CAP ? ref == (TB_PKREF_READY | r) : ref == TB_PKREF_NONE);
    }
    std::vector<uint8_t> none;  // a cap of 0: nothing is ever marked
    comb_mark_ready(none.data(), 0, 0);
    CHECK(comb_ref(true, 7, true) == (TB_PKREF_READY | TB_PKREF_TABLE | 7u));
    CHECK((comb_ref(true, 0x3fffffffu, true) & TB_PKREF_ROW) == 0x3fffffffu);
    CHECK(comb_ref(true, 7, false) == TB_PKREF_NONE && !(TB_PKREF_NONE & TB_PKREF_READY));
  }

  printf("keys %zu scalars %zu\n", keys.size(), rs.size());
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
