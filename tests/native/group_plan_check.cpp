// CPU check of the grouped batch plan (teku_amd/csrc/tb_plan.h;
// tests/test_group_host.py).  Prints one line per failed check, then
// `ok <checks>` when none failed (exit status 1 otherwise):
//   * n_msgs == n (and the default) gives the plan and the workspace layout of
//     today, field for field, over plan_check.cpp's size sweep, every key
//     source and the settle plan;
//   * a grouped plan has n_msgs + 64 pairs, the bucket-sum signature side,
//     kernels chosen by n_msgs (hash, lines, wave / split, product levels) and
//     by n (w2, key stage), per-set regions of n items and per-pair regions of
//     n_pairs, no two regions overlapping, and is never settle_ready;
//   * group_plan (behind tbls_group_plan) agrees with group_pays and the plan
//     on both sides of group_min / percent, from plan_env values set here.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "tb_plan.h"

using namespace tb;
using namespace tb::plan;

static long g_checks = 0, g_failed = 0;
#define CHECK(c, ...)                           \
  do {                                          \
    g_checks++;                                 \
    if (!(c)) {                                 \
      g_failed++;                               \
      printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                      \
      printf("\n");                             \
    }                                           \
  } while (0)

static const uint32_t SIZES[] = {0, 1, 2, 3, 4, 5, 16, 17, 64, 128, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
                                 8191, 8192, 8193, 16383, 16384, 16385, 20479, 20480, 20481, 32767, 32768, 32769, 40000, 65535, 65536, 65537,
                                 131071, 131072, 131073, 262143, 262144, 262145, 300000, 524288, 1048576};
struct source {
  key_source src;
  uint32_t keys_per_set;
};
static const source SOURCES[] = {{key_source::bytes, 1}, {key_source::table, 1}, {key_source::bits, 1}, {key_source::bytes, 2}};

static bool same_pairs(const pair_plan& a, const pair_plan& b) {
  return a.n == b.n && a.n_msgs == b.n_msgs && a.n_extra == b.n_extra && a.n_pairs == b.n_pairs && a.n_main == b.n_main && a.n_xwave == b.n_xwave &&
         a.per == b.per && a.nseg == b.nseg && a.grouped == b.grouped && a.msm == b.msm && a.wave == b.wave && a.split == b.split;
}
static bool same_plan(const batch_plan& a, const batch_plan& b) {
  if (!same_pairs(a.pp, b.pp) || a.n_keys != b.n_keys || a.hash != b.hash || a.sig != b.sig || a.key != b.key || a.w2 != b.w2 || a.multi != b.multi ||
      a.line_group != b.line_group || a.late_join != b.late_join || a.sig_first != b.sig_first || a.prod_chunk != b.prod_chunk ||
      a.n_levels != b.n_levels || a.combine != b.combine)
    return false;
  for (int i = 0; i < a.n_levels; i++) {
    const prod_level &x = a.levels[i], &y = b.levels[i];
    if (x.seg != y.seg || x.n_in != y.n_in || x.n_in_last != y.n_in_last || x.in_stride != y.in_stride || x.chunk != y.chunk || x.n_out != y.n_out ||
        x.out_stride != y.out_stride || x.dst != y.dst)
      return false;
  }
  return true;
}
static std::vector<size_t> offsets(const ws_layout& L) {
  return {L.pk_aff, L.pk_code, L.P, L.Q, L.skip, L.set_code, L.sig_code, L.pair_code, L.sig_aff, L.sig_use, L.msm_cnt, L.msm_off, L.msm_cur, L.msm_idx,
          L.msm_sum, L.mlist, L.mcnt, L.hrow, L.lines, L.f, L.fpart, L.fpart2, L.segv, L.n_bad, L.result, L.set_P, L.grp_item, L.grp_part,
          L.grp_pskip, L.total};
}

// the ungrouped layout as tb_plan.h stated it before grouped plans (kept here
// in full, so a change to an ungrouped offset fails)
static std::vector<size_t> layout_of_today(const batch_plan& bp, size_t& code_bytes) {
  const pair_plan& pp = bp.pp;
  const uint32_t n = pp.n, np = pp.n_pairs, nf = pp.n_f(), K = bp.n_keys, pc = bp.prod_chunk;
  const bool msm = pp.msm;
  const uint32_t nb_f = (nf + pc - 1) / pc + pp.nseg * ((pp.n_groups() + pp.n_xwave + TB_PROD_CHUNK - 1) / TB_PROD_CHUNK);
  std::vector<size_t> v;
  size_t o = 0;
  const auto reg = [&](size_t bytes) {
    v.push_back(o);
    o = align_up(o + bytes);
  };
  reg((size_t)K * sizeof(g1a));  // pk_aff
  reg(K);                        // pk_code
  reg((size_t)np * sizeof(g1a)); // P
  reg((size_t)np * sizeof(g2a)); // Q
  reg(np);                       // skip
  reg(np);                       // set_code
  reg(np);                       // sig_code
  code_bytes = 2 * align_up(np);
  v.push_back(o);                // pair_code: empty
  const size_t nm = msm ? n : 0;
  reg(nm * sizeof(g2a));         // sig_aff
  reg(nm);                       // sig_use
  reg(msm ? TB_MSM_BUCKETS * 4 : 0);
  reg(msm ? (TB_MSM_BUCKETS + 1) * 4 : 0);
  reg(msm ? TB_MSM_BUCKETS * 4 : 0);
  reg(nm * 8 * 4);               // msm_idx
  reg(msm ? (size_t)TB_MSM_BUCKETS * sizeof(g2j) : 0);
  reg((size_t)n * 4);            // mlist
  reg(4);                        // mcnt
  reg(bp.hash == hash_kind::row ? (size_t)n * HROW_SET_BYTES : 0);
  reg(std::max((size_t)pp.line_pairs() * LINE_BYTES_PER_PAIR, bp.hash == hash_kind::w2 ? (size_t)n * sizeof(g2a) : 0));
  reg((size_t)(nf ? nf : 1) * sizeof(fp12));
  reg((size_t)nb_f * sizeof(fp12));
  reg((size_t)((nb_f + pc - 1) / pc + pp.nseg) * sizeof(fp12));
  reg((size_t)pp.nseg * sizeof(fp12));
  reg(4);                        // n_bad
  reg(4);                        // result
  for (int i = 0; i < 4; i++) v.push_back(o);  // set_P, grp_item, grp_part, grp_pskip: empty
  v.push_back(o);                // total
  return v;
}

static void check_ungrouped(const plan_env& env) {
  for (uint32_t n : SIZES)
    for (const source& s : SOURCES)
      for (int settle = 0; settle < 2; settle++) {
        const batch_plan two(n, s.keys_per_set * n, s.src, settle != 0, env);
        for (uint32_t nm : {n, 0u, n + 1u}) {  // n itself, the default, and past n
          const batch_plan bp(n, s.keys_per_set * n, s.src, settle != 0, env, nm);
          CHECK(same_plan(two, bp), "n=%u n_msgs=%u settle=%d", n, nm, settle);
          CHECK(!bp.pp.grouped && bp.pp.n_msgs == n && bp.pp.x_first() == n, "n=%u", n);
          size_t cb = 0;
          const ws_layout L(bp);
          CHECK(offsets(L) == offsets(ws_layout(two)) && offsets(L) == layout_of_today(two, cb), "n=%u n_msgs=%u settle=%d", n, nm, settle);
          CHECK(L.code_bytes == cb, "n=%u", n);
        }
        // the settle plan ignores groups
        if (settle && n > 1) CHECK(same_plan(two, batch_plan(n, s.keys_per_set * n, s.src, true, env, 1u)), "n=%u", n);
        CHECK(settle_ready(n, env) == settle_ready(n, env, n), "n=%u", n);
      }
}

static void check_grouped(const plan_env& env) {
  for (uint32_t n : SIZES)
    for (uint32_t m : {1u, 2u, 8u, 64u, 448u, 449u, 512u, 513u, 1024u, 1025u, 1984u, 1985u, 2048u, 8192u, 8193u, 32768u, 32769u, n / 64u, n / 2u, n - 1u}) {
      if (!m || m >= n) continue;
      for (const source& s : SOURCES) {
        const batch_plan bp(n, s.keys_per_set * n, s.src, false, env, m);
        const pair_plan& pp = bp.pp;
        CHECK(pp.grouped && pp.n == n && pp.n_msgs == m && pp.x_first() == m, "n=%u m=%u", n, m);
        CHECK(pp.n_pairs == m + 64u && pp.n_extra == TB_MSM_XPAIRS, "n=%u m=%u pairs=%u", n, m, pp.n_pairs);
        CHECK(pp.msm && bp.sig == sig_kind::msm, "n=%u m=%u", n, m);
        CHECK(!settle_ready(n, env, m), "n=%u m=%u", n, m);
        // by m: the plan of an ungrouped bucket-sum batch of m sets has the same pairs, hash and product tree
        plan_env msm_env = env;
        msm_env.msm_min = 0;
        const batch_plan by_m(m, m, s.src, false, msm_env);
        CHECK(pp.wave == by_m.pp.wave && pp.split == by_m.pp.split && pp.n_main == by_m.pp.n_main && pp.n_xwave == by_m.pp.n_xwave &&
                  pp.per == by_m.pp.per && pp.nseg == by_m.pp.nseg && pp.n_f() == by_m.pp.n_f(),
              "n=%u m=%u", n, m);
        CHECK(pp.wave == (m + 64u <= env.miller_wave_max), "n=%u m=%u", n, m);
        CHECK(bp.hash == by_m.hash && bp.line_group == by_m.line_group && bp.prod_chunk == by_m.prod_chunk && bp.n_levels == by_m.n_levels &&
                  bp.combine == by_m.combine,
              "n=%u m=%u", n, m);
        for (int i = 0; i < bp.n_levels; i++)
          CHECK(bp.levels[i].n_in == by_m.levels[i].n_in && bp.levels[i].n_out == by_m.levels[i].n_out && bp.levels[i].dst == by_m.levels[i].dst,
                "n=%u m=%u level %d", n, m, i);
        // by n: the per-set kernels
        const batch_plan by_n(n, s.keys_per_set * n, s.src, false, env);
        CHECK(bp.w2 == by_n.w2 && bp.key == by_n.key && bp.multi == by_n.multi && bp.n_keys == by_n.n_keys && bp.sig_first == by_n.sig_first,
              "n=%u m=%u", n, m);
        // the workspace: sizes from the next region's start, no overlap
        const ws_layout L(bp);
        const uint32_t np = pp.n_pairs, ni = group_items_max(n, m);
        std::vector<std::pair<size_t, size_t>> reg = {
            {L.pk_aff, (size_t)bp.n_keys * sizeof(g1a)}, {L.pk_code, bp.n_keys},
            {L.P, (size_t)np * sizeof(g1a)}, {L.Q, (size_t)np * sizeof(g2a)}, {L.skip, np},  // per pair
            {L.set_code, n}, {L.sig_code, n},                                               // per set
            {L.pair_code, 2 * align_up(np)},                                                // two rows per pair
            {L.sig_aff, (size_t)n * sizeof(g2a)}, {L.sig_use, n}, {L.msm_cnt, TB_MSM_BUCKETS * 4}, {L.msm_off, (TB_MSM_BUCKETS + 1) * 4},
            {L.msm_cur, TB_MSM_BUCKETS * 4}, {L.msm_idx, (size_t)n * 32}, {L.msm_sum, (size_t)TB_MSM_BUCKETS * sizeof(g2j)},
            {L.mlist, (size_t)n * 4}, {L.mcnt, 4},
            {L.hrow, bp.hash == hash_kind::row ? (size_t)m * HROW_SET_BYTES : 0},
            {L.lines, std::max((size_t)pp.line_pairs() * LINE_BYTES_PER_PAIR, bp.hash == hash_kind::w2 ? (size_t)m * sizeof(g2a) : 0)},
            {L.f, (size_t)std::max(pp.n_f(), 1u) * sizeof(fp12)}, {L.fpart, (size_t)L.nb_f * sizeof(fp12)}, {L.segv, (size_t)pp.nseg * sizeof(fp12)},
            {L.n_bad, 4}, {L.result, 4},
            {L.set_P, (size_t)n * sizeof(g1a)},  // per set
            {L.grp_item, ((size_t)m + 1) * 4}, {L.grp_part, (size_t)ni * sizeof(g1a)}, {L.grp_pskip, ni}};
        reg.push_back({L.fpart2, 0});  // its size is the layout's business; it must lie between fpart and segv
        std::sort(reg.begin(), reg.end());
        bool ok = true;
        for (size_t i = 0; i < reg.size(); i++) {
          ok = ok && reg[i].first % 256 == 0 && reg[i].first + reg[i].second <= L.total;
          if (i + 1 < reg.size()) ok = ok && reg[i].first + reg[i].second <= reg[i + 1].first;
        }
        CHECK(ok, "n=%u m=%u: regions overlap or leave the workspace", n, m);
        CHECK(L.code_bytes == L.pair_code + 2 * align_up(np) - L.set_code && L.sig_code >= L.set_code + n && L.pair_code >= L.sig_code + n,
              "n=%u m=%u: the zeroed code rows", n, m);
        // the items of the group sums: a walk covers n in one round of the chip's rows, and the bound holds for any split of n into m groups
        const uint32_t walk = group_walk(n);
        CHECK(walk % TB_GROUP_ROWS == 0 && walk >= TB_GROUP_ROWS * TB_GROUP_WALK_MIN && (uint64_t)walk * 256u >= n, "n=%u walk=%u", n, walk);
        const uint32_t big = n - (m - 1);  // one group as large as it can be, the others single
        CHECK((big + walk - 1) / walk + (m - 1) <= ni, "n=%u m=%u", n, m);
      }
    }
}

static void check_thresholds() {
  plan_env env;
  int g = -1;
  uint32_t np = 0;
  // the built-in default: measured thresholds or never -- whichever, force groups and m == n does not
  group_plan(4096, 64, g, np, env);
  CHECK(g >= 1 && np == 128u, "default: grouped=%d pairs=%u", g, np);
  CHECK(group_pays(4096, 64, true, env) && !group_pays(4096, 4096, true, env) && !group_pays(4096, 0, true, env) && !group_pays(0, 0, true, env), "force");
  env.parse_group_min("1000,25");
  CHECK(env.group_min == 1000u && env.group_percent == 25u, "parse");
  struct {
    uint32_t n, m;
    int grouped;
  } cases[] = {{999, 10, 1},   {1000, 10, 2},  {1000, 250, 2}, {1000, 251, 1}, {1000, 999, 1}, {1000, 1000, 0},
               {1000, 1001, 0}, {1000, 0, 0},   {4096, 1024, 2}, {4096, 1025, 1}, {1, 1, 0},      {2, 1, 1},      {0, 0, 0}};
  for (const auto& c : cases) {
    group_plan(c.n, c.m, g, np, env);
    CHECK(g == c.grouped, "n=%u m=%u grouped=%d", c.n, c.m, g);
    CHECK((g == 2) == group_pays(c.n, c.m, false, env) && (g >= 1) == group_pays(c.n, c.m, true, env), "n=%u m=%u", c.n, c.m);
    CHECK(np == pair_plan(c.n, false, env, g ? c.m : 0u).n_pairs && (!g || np == c.m + 64u), "n=%u m=%u pairs=%u", c.n, c.m, np);
    CHECK(g || np == pair_plan(c.n, false, env).n_pairs, "n=%u m=%u", c.n, c.m);
  }
  env.parse_group_min("0");
  CHECK(env.group_min == 0u && env.group_percent == 25u && group_pays(2, 1, false, env) == (100u <= 25u * 2u), "min only");
  env.parse_group_min("5,101");  // a percent past 100 is not taken
  CHECK(env.group_min == 5u && env.group_percent == 25u, "percent bound");
  env.parse_group_min(nullptr);
  CHECK(env.group_min == 5u, "unset keeps");
}

int main() {
  plan_env def;  // the built-in defaults, whatever the caller's environment holds
  check_ungrouped(def);
  check_grouped(def);
  plan_env tuned = def;
  tuned.parse_miller_wave_max("256");
  tuned.parse_hash_plan("600,0,3000");
  tuned.parse_coop("0");
  check_ungrouped(tuned);
  check_grouped(tuned);
  check_thresholds();
  if (g_failed) {
    printf("%ld of %ld checks failed\n", g_failed, g_checks);
    return 1;
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
