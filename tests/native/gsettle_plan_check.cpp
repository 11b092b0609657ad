// CPU check of the scratch layout of settling a failed grouped batch
// (teku_amd/csrc/tb_plan.h gsettle_layout; tests/test_gsettle_plan.py), a
// stand-alone program.  Prints one line per failed check, then `ok <checks>`
// when none failed (exit status 1 otherwise).  Over n sets, m messages and the
// default and a 256-position chunk:
//   * the regions are disjoint, 256-byte aligned, inside `total`, and each is
//     as large as its contents (stated here from the element sizes);
//   * the chunks cover [0, n) exactly once, none empty, none above `chunk`;
//   * the tail's nseg / nA / nB and the sizes of its V / A / B / list / out
//     are settle_layout(n)'s;
//   * the verdicts' position-to-set map, the CSR of tb_group.h group_messages,
//     is a permutation of [0, n) whose positions lie inside their message's
//     range, on interleaved and on sorted inputs;
//   * TBLS_GSETTLE_CHUNK parses as plan_env says (a value of 0 or past
//     TB_LINE_CHUNK keeps the default).
#include <algorithm>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "tb_group.h"
#include "tb_plan.h"

using namespace tb;
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

struct msg_set {
  const uint8_t* msg;
  uint32_t msg_len;
};

static void check_layout(uint32_t n, uint32_t m, const plan_env& env, uint32_t want_chunk) {
  const gsettle_layout S(n, m, env);
  const settle_layout R(n);
  CHECK(S.n == n && S.m == m, "n %u m %u", n, m);
  CHECK(S.chunk == std::min(n, want_chunk), "n %u chunk %u want %u", n, S.chunk, std::min(n, want_chunk));
  const settle_layout& T = S.tail;
  CHECK(T.n == n && T.nseg == R.nseg && T.nA == R.nA && T.nB == R.nB, "n %u: %u/%u/%u vs %u/%u/%u", n, T.nseg, T.nA, T.nB, R.nseg, R.nA, R.nB);
  // the regions with their contents' sizes: 68 lines of 288 B per column, 576-byte Fp12 values, 96-byte G1 and 192-byte G2 points
  const size_t LINE = 68u * 288u, F12 = 576;
  CHECK(sizeof(fp12) == F12 && sizeof(g1a) == 96 && sizeof(g2a) == 192 && LINE_BYTES_PER_PAIR == LINE, "type sizes");
  const std::pair<size_t, size_t> reg[] = {
      {S.mlines, (size_t)m * LINE},       {S.msg_of_pos, (size_t)n * 4},      {S.negr, (size_t)S.chunk * 96}, {S.sigq, (size_t)S.chunk * 192},
      {S.sskip, (size_t)S.chunk},         {S.slines, (size_t)S.chunk * LINE}, {T.V, (size_t)T.nseg * n * F12}, {T.A, (size_t)T.nseg * T.nA * F12},
      {T.B, (size_t)T.nseg * T.nB * F12}, {T.list, (size_t)n * 4},            {T.out, (size_t)n}};
  const size_t NR = sizeof(reg) / sizeof(reg[0]);
  for (size_t a = 0; a < NR; a++) {
    CHECK(reg[a].first % 256 == 0, "n %u m %u region %zu at %zu", n, m, a, reg[a].first);
    CHECK(reg[a].first + reg[a].second <= S.total, "n %u m %u region %zu ends past total", n, m, a);
    for (size_t b = a + 1; b < NR; b++)
      CHECK(reg[a].first + reg[a].second <= reg[b].first || reg[b].first + reg[b].second <= reg[a].first, "n %u m %u regions %zu and %zu overlap", n, m,
            a, b);
  }
  CHECK(T.A - T.V == R.A - R.V && T.B - T.A == R.B - R.A && T.list - T.B == R.list - R.B && T.out - T.list == R.out - R.list &&
            S.total - T.out == R.total - R.out && T.total == S.total,
        "n %u: the tail regions' sizes differ from settle_layout's", n);
  // the chunks
  uint64_t next = 0;
  for (uint32_t k = 0; k < S.n_chunks; k++) {
    CHECK(S.lo(k) == next, "n %u chunk %u starts at %u, want %llu", n, k, S.lo(k), (unsigned long long)next);
    CHECK(S.hi(k) > S.lo(k) && S.hi(k) - S.lo(k) <= S.chunk, "n %u chunk %u [%u, %u)", n, k, S.lo(k), S.hi(k));
    next = S.hi(k);
  }
  CHECK(next == n, "n %u: the chunks end at %llu", n, (unsigned long long)next);
  // the line kernel of a chunk: one wave round of lane groups at most (tb_plan.h line_group)
  const int lg = line_group(S.chunk, env);
  CHECK(lg == 1 || (uint64_t)lg * S.chunk <= TB_GROUP_LANES, "n %u line group %d", n, lg);
}

// n sets over m messages, interleaved (set i signs message i mod m) or sorted
// (message by message, floor(i m / n)); every message has a set
static void check_positions(uint32_t n, uint32_t m, bool sorted) {
  std::vector<std::string> text(m);
  for (uint32_t g = 0; g < m; g++) text[g] = "message " + std::to_string(g);
  std::vector<msg_set> sets(n);
  std::vector<uint32_t> want(n);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t g = sorted ? (uint32_t)((uint64_t)i * m / n) : i % m;
    want[i] = g;
    sets[i] = {(const uint8_t*)text[g].data(), (uint32_t)text[g].size()};
  }
  const group::groups G = group::group_messages(sets.data(), 0, n);
  CHECK(G.m == m, "n %u m %u sorted %d: %u groups", n, m, (int)sorted, G.m);
  CHECK(G.grp_off.size() == (size_t)G.m + 1 && G.grp_off[0] == 0 && G.grp_off[G.m] == n && G.grp_sets.size() == n, "n %u m %u CSR shape", n, m);
  if (G.m != m || G.grp_sets.size() != n) return;
  // ok[grp_sets[t]] = verdict of position t must write every set exactly once
  std::vector<uint8_t> seen(n, 0);
  long dup = 0, wrong = 0;
  for (uint32_t g = 0; g < m; g++)
    for (uint32_t t = G.grp_off[g]; t < G.grp_off[g + 1]; t++) {
      const uint32_t i = G.grp_sets[t];
      if (i >= n || seen[i]++) {
        dup++;
        continue;
      }
      if (want[i] != g) wrong++;  // both inputs number the messages by first appearance
    }
  CHECK(dup == 0 && wrong == 0, "n %u m %u sorted %d: %ld repeated or out of range, %ld in another message's range", n, m, (int)sorted, dup, wrong);
  CHECK((uint32_t)std::count(seen.begin(), seen.end(), 1) == n, "n %u m %u: not every set has a position", n, m);
}

int main() {
  const uint32_t NS[] = {1, 2, 15, 16, 17, 255, 256, 257, 828, 2304, 131072, 131073, 300000};
  for (uint32_t n : NS) {
    const uint32_t MS[] = {1, 2, n / 2, n - 1};
    for (uint32_t m : MS) {
      if (m < 1 || m > n) continue;
      plan_env dflt, small;
      small.parse_gsettle_chunk("256");
      CHECK(dflt.gsettle_chunk == TB_SETTLE_MAX && small.gsettle_chunk == 256, "chunk defaults");
      check_layout(n, m, dflt, TB_SETTLE_MAX);
      check_layout(n, m, small, 256);
      check_positions(n, m, false);
      check_positions(n, m, true);
    }
  }
  {
    plan_env e;
    e.parse_gsettle_chunk(nullptr);
    CHECK(e.gsettle_chunk == TB_SETTLE_MAX, "unset");
    e.parse_gsettle_chunk("0");
    CHECK(e.gsettle_chunk == TB_SETTLE_MAX, "0 keeps the default");
    e.parse_gsettle_chunk("999999999");
    CHECK(e.gsettle_chunk == TB_SETTLE_MAX, "past TB_LINE_CHUNK keeps the default");
    e.parse_gsettle_chunk("4096");
    CHECK(e.gsettle_chunk == 4096, "4096");
  }
  if (g_failed) {
    printf("%ld of %ld checks failed\n", g_failed, g_checks);
    return 1;
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
