// CPU check of the group-test descent of settling a failed batch
// (teku_amd/csrc/tb_settle.h settle_descent; tests/test_settle_descent.py), a
// stand-alone program.  Prints one line per failed check, then `ok <checks>`
// when none failed (exit status 1 otherwise).  The tester is simulated: value i
// is 1 unless set i is invalid and its code is 0 (a coded set's value is 1, as
// k_settle_mask arranges on the device), and a group passes iff every value
// in it is 1.  Over n = 1, 15, 16, 17, 255, 256, 257, 4097 sets (the edges of
// the fan-out of 16: at 257, nA = 17 and nB = 2), three code arrays (no coded
// set, every seventh, all) and these invalid sets -- none; the first, the last,
// a middle one; one in every level-A group of the first and of the last
// level-B group; all; exactly the coded ones:
//   * the verdicts are codes[i] == 0 && !invalid[i];
//   * the tester never sees an empty list, sees the levels in the order B, A,
//     leaves, each at most once, and every list strictly ascending;
//   * every level-A index it sees is a child of a failing level-B group;
//   * every leaf it sees has code 0 and a failing level-A group;
//   * the number of groups tested is the one counted from the pattern: all
//     level-B groups, the children of the failing ones, and the code-0 members
//     of the failing level-A groups.
// And an error code from the tester ends the descent and is returned.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "tb_settle.h"

using namespace tb::plan;

static long g_checks = 0, g_failed = 0;
#define CHECK(c, ...)                                      \
  do {                                                     \
    g_checks++;                                            \
    if (!(c)) {                                            \
      g_failed++;                                          \
      printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                                 \
      printf("\n");                                        \
    }                                                      \
  } while (0)

static const uint32_t F = TB_SETTLE_FAN;

// the values of one case: bad[i] = value i is not 1
struct sim {
  uint32_t n;
  std::vector<uint8_t> bad;
  // members of index g of `level`: [lo, hi)
  uint32_t lo(int level, uint32_t g) const { return level == SETTLE_B ? g * F * F : level == SETTLE_A ? g * F : g; }
  uint32_t hi(int level, uint32_t g) const {
    const uint64_t w = level == SETTLE_B ? F * F : level == SETTLE_A ? F : 1;
    return (uint32_t)std::min<uint64_t>(n, (g + 1) * w);
  }
  bool passes(int level, uint32_t g) const {
    for (uint32_t i = lo(level, g); i < hi(level, g); i++)
      if (bad[i]) return false;
    return true;
  }
};

static void check_case(uint32_t n, const std::vector<uint8_t>& codes, const std::vector<uint8_t>& invalid, const char* what) {
  const settle_layout S(n);
  sim v{n, std::vector<uint8_t>(n)};
  for (uint32_t i = 0; i < n; i++) v.bad[i] = invalid[i] && codes[i] == 0;
  // the groups the descent has to test, counted from the pattern
  size_t want_tested = S.nB;
  for (uint32_t b = 0; b < S.nB; b++)
    if (!v.passes(SETTLE_B, b)) want_tested += std::min(S.nA, (b + 1) * F) - b * F;
  for (uint32_t a = 0; a < S.nA; a++)
    if (!v.passes(SETTLE_A, a))
      for (uint32_t i = v.lo(SETTLE_A, a); i < v.hi(SETTLE_A, a); i++) want_tested += codes[i] == 0;

  size_t tested = 0;
  int last_level = SETTLE_B + 1;
  std::vector<uint8_t> ok(n, 2);
  const int rc = settle_descent(S, codes, ok.data(), [&](settle_level level, const std::vector<uint32_t>& list, std::vector<uint8_t>& pass) {
    CHECK(!list.empty(), "n %u %s: empty list at level %d", n, what, (int)level);
    CHECK((int)level < last_level, "n %u %s: level %d after level %d", n, what, (int)level, last_level);
    last_level = level;
    CHECK(pass.size() == list.size(), "n %u %s: %zu verdict bytes for %zu entries", n, what, pass.size(), list.size());
    const uint32_t count = level == SETTLE_B ? S.nB : level == SETTLE_A ? S.nA : n;
    long unordered = 0, outside = 0, stray = 0;
    for (size_t k = 0; k < list.size(); k++) {
      const uint32_t g = list[k];
      if (k && list[k - 1] >= g) unordered++;
      if (g >= count) {
        outside++;
        continue;
      }
      if (level == SETTLE_A && v.passes(SETTLE_B, g / F)) stray++;
      if (level == SETTLE_LEAF && (codes[g] != 0 || v.passes(SETTLE_A, g / F))) stray++;
      pass[k] = v.passes(level, g);
    }
    CHECK(unordered == 0 && outside == 0, "n %u %s level %d: %ld entries out of order, %ld out of range", n, what, (int)level, unordered, outside);
    CHECK(level != SETTLE_B || list.size() == S.nB, "n %u %s: %zu of %u level-B groups", n, what, list.size(), S.nB);
    CHECK(stray == 0, "n %u %s level %d: %ld entries coded or under a passing group", n, what, (int)level, stray);
    tested += list.size();
    return 0;
  });
  CHECK(rc == 0, "n %u %s: rc %d", n, what, rc);
  long wrong = 0;
  for (uint32_t i = 0; i < n; i++) wrong += ok[i] != (codes[i] == 0 && !invalid[i] ? 1 : 0);
  CHECK(wrong == 0, "n %u %s: %ld wrong verdicts", n, what, wrong);
  CHECK(tested == want_tested, "n %u %s: %zu groups tested, want %zu", n, what, tested, want_tested);
}

int main() {
  const uint32_t NS[] = {1, 15, 16, 17, 255, 256, 257, 4097};
  for (uint32_t n : NS) {
    const settle_layout S(n);
    CHECK(S.nA == (n + F - 1) / F && S.nB == (S.nA + F - 1) / F, "n %u: nA %u nB %u", n, S.nA, S.nB);
    if (n == 257) CHECK(S.nA == 17 && S.nB == 2, "n 257: nA %u nB %u", S.nA, S.nB);
    std::vector<std::vector<uint8_t>> code_sets(3, std::vector<uint8_t>(n, 0));
    for (uint32_t i = 0; i < n; i++) {
      if (i % 7 == 3) code_sets[1][i] = 3;
      code_sets[2][i] = 1 + i % 5;
    }
    for (const std::vector<uint8_t>& codes : code_sets) {
      std::vector<uint8_t> inv(n, 0);
      check_case(n, codes, inv, "no failure");
      for (uint32_t at : {0u, n - 1, n / 2}) {
        inv.assign(n, 0);
        inv[at] = 1;
        check_case(n, codes, inv, at == 0 ? "first fails" : at == n - 1 ? "last fails" : "middle fails");
      }
      for (uint32_t b : {0u, S.nB - 1}) {  // one failure in every level-A group of level-B group b, not at the groups' first member
        inv.assign(n, 0);
        for (uint32_t a = b * F; a < std::min(S.nA, (b + 1) * F); a++) inv[std::min(n - 1, a * F + a % F)] = 1;
        check_case(n, codes, inv, b == 0 ? "every A group of the first B group fails" : "every A group of the last B group fails");
      }
      inv.assign(n, 1);
      check_case(n, codes, inv, "all fail");
      for (uint32_t i = 0; i < n; i++) inv[i] = codes[i] != 0;
      check_case(n, codes, inv, "the coded sets fail");
    }
  }
  {  // the tester's error ends the descent
    const uint32_t n = 257;
    const settle_layout S(n);
    const std::vector<uint8_t> codes(n, 0);
    std::vector<uint8_t> ok(n, 2);
    int calls = 0;
    const int rc = settle_descent(S, codes, ok.data(), [&](settle_level level, const std::vector<uint32_t>&, std::vector<uint8_t>&) {
      calls++;
      return level == SETTLE_A ? -7 : 0;  // every level-B group fails (pass stays 0), then the error
    });
    CHECK(rc == -7 && calls == 2, "rc %d after %d calls", rc, calls);
  }
  if (g_failed) {
    printf("%ld of %ld checks failed\n", g_failed, g_checks);
    return 1;
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
