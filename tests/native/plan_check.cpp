// CPU check of the batch plan (teku_amd/csrc/tb_plan.h; tests/test_batch_plan.py).
//   plan_check dump    one line per (sets, key source, settle): every decision
//                      of batch_plan, pair_plan's counts, the product levels
//                      and the workspace size, under the process environment
//                      (compared with tests/golden/batch_plan.txt)
//   plan_check check   the plan's invariants at the same sizes under the
//                      default settings and the overrides the GPU tests use,
//                      and the settle scratch layout's up to TB_SETTLE_MAX sets
#include <cstring>
#include <string>

#include "tb_plan.h"

using namespace tb::plan;

// the sizes at which a decision flips under default settings, with their neighbours
static const uint32_t SIZES[] = {0, 1, 2, 3, 4, 5, 16, 17, 64, 128, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
                                 8191, 8192, 8193, 16383, 16384, 16385, 20479, 20480, 20481, 32767, 32768, 32769, 40000, 65535, 65536, 65537,
                                 131071, 131072, 131073, 262143, 262144, 262145, 300000, 524288, 1048576};

// key sources of the sweep: bytes / table / bits with one key per set, and
// bytes with two keys per set (the multi-key aggregation)
struct source {
  const char* name;
  key_source src;
  uint32_t keys_per_set;
};
static const source SOURCES[] = {{"bytes", key_source::bytes, 1}, {"table", key_source::table, 1}, {"bits", key_source::bits, 1}, {"bytes2", key_source::bytes, 2}};

static const char* HASH[] = {"none", "coop", "wave", "row", "quad", "duo", "w2", "lane"};
static const char* SIG[] = {"msm", "coop", "pair"};
static const char* KEY[] = {"bits", "keys_coop", "table", "decompress"};
static const char* DST[] = {"fpart", "fpart2", "segv", "partial"};

template <class FN>
static void sweep(const plan_env& env, FN fn) {
  for (uint32_t n : SIZES)
    for (const source& s : SOURCES)
      for (int settle = 0; settle < 2; settle++) {
        if (s.keys_per_set > 1 && settle) continue;
        fn(n, s, settle != 0, batch_plan(n, s.keys_per_set * n, s.src, settle != 0, env));
      }
}

static void dump(uint32_t n, const source& s, bool settle, const batch_plan& bp) {
  const pair_plan& pp = bp.pp;
  const bool sig_w2 = bp.w2 && bp.sig != sig_kind::coop;
  printf("n=%u src=%s settle=%d hash=%s sig=%s%s key=%s multi=%u pk_w2=%d lg=%d late=%d sf=%d pc=%u", n, s.name, (int)settle, HASH[(int)bp.hash],
         SIG[(int)bp.sig], sig_w2 ? "+w2" : "", KEY[(int)bp.key], bp.multi, (int)bp.w2, bp.line_group, (int)bp.late_join, bp.sig_first, bp.prod_chunk);
  printf(" msm=%d wave=%d split=%d seg=%d extra=%u pairs=%u main=%u xwave=%u per=%u nseg=%u groups=%u nf=%u lines=%u one=%d", (int)pp.msm,
         (int)pp.wave, (int)pp.split, (int)pp.seg(), pp.n_extra, pp.n_pairs, pp.n_main, pp.n_xwave, pp.per, pp.nseg, pp.n_groups(), pp.n_f(),
         pp.line_pairs(), (int)(pp.n_f() == 0));
  printf(" levels=");
  if (!bp.n_levels) printf("-");
  for (int i = 0; i < bp.n_levels; i++) {
    const prod_level& l = bp.levels[i];
    if (l.seg)
      printf("s:%u/%u/%u/%u@%ux%u>%s/%u,", l.n_in, l.n_in_last, l.in_stride, l.chunk, l.n_out, pp.nseg, DST[(int)l.dst], l.out_stride);
    else
      printf("w:%u/%u@%u>%s%s", l.n_in, l.chunk, l.n_out, DST[(int)l.dst], i + 1 < bp.n_levels ? "," : "");
  }
  if (bp.combine) printf("combine>partial");
  printf(" total=%zu\n", ws_layout(bp).total);
}

static int g_fail = 0;
static std::string g_where;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      g_fail++;                                                       \
      printf("FAIL %s: %s (line %d)\n", g_where.c_str(), #c, __LINE__); \
    }                                                                 \
  } while (0)

static void check(uint32_t n, const source& s, bool settle, const batch_plan& bp, const char* env_name) {
  g_where = std::string(env_name) + " n=" + std::to_string(n) + " src=" + s.name + " settle=" + std::to_string((int)settle);
  const pair_plan& pp = bp.pp;
  const ws_layout L(bp);
  // regions: 256-byte aligned, increasing, covered by total.  Each region ends
  // where the next begins, so "increasing" is "pairwise disjoint".
  const size_t off[] = {L.pk_aff, L.pk_code, L.P, L.Q, L.skip, L.set_code, L.sig_code, L.sig_aff, L.sig_use, L.msm_cnt, L.msm_off, L.msm_cur, L.msm_idx,
                        L.msm_sum, L.mlist, L.mcnt, L.hrow, L.lines, L.f, L.fpart, L.fpart2, L.segv, L.n_bad, L.result, L.total};
  const int R = (int)(sizeof(off) / sizeof(off[0]));
  CHECK(off[0] == 0);
  for (int i = 0; i < R; i++) CHECK(off[i] % 256 == 0);
  for (int i = 0; i + 1 < R; i++) CHECK(off[i] <= off[i + 1]);
  CHECK(L.total >= L.result + 4 && L.result >= L.n_bad + 4);
  // what the stages write fits its region
  CHECK(L.Q - L.P >= (size_t)pp.n_pairs * sizeof(tb::g1a) && L.skip - L.Q >= (size_t)pp.n_pairs * sizeof(tb::g2a));
  CHECK(L.sig_code == L.set_code + align_up(pp.n_pairs) && L.sig_aff - L.sig_code >= pp.n_pairs);  // one memset clears both code rows
  CHECK(L.fpart - L.f >= (size_t)(pp.n_f() ? pp.n_f() : 1) * sizeof(tb::fp12));
  CHECK(L.n_bad - L.segv >= (size_t)pp.nseg * sizeof(tb::fp12));
  CHECK(L.f - L.lines >= (size_t)pp.line_pairs() * LINE_BYTES_PER_PAIR);
  if (bp.hash == hash_kind::row) CHECK(L.lines - L.hrow >= (size_t)n * HROW_SET_BYTES);
  if (pp.msm) CHECK(L.sig_use - L.sig_aff >= (size_t)n * sizeof(tb::g2a) && L.mlist - L.msm_sum >= (size_t)TB_MSM_BUCKETS * sizeof(tb::g2j));
  // the w2 hash's park area (a g2a per set) lies inside `lines`, which ends before f
  if (bp.hash == hash_kind::w2) CHECK(L.lines + (size_t)n * 192 <= L.f);
  CHECK(L.lines + (size_t)pp.line_pairs() * LINE_BYTES_PER_PAIR <= L.f);
  // one kind per stage
  if (n) {
    CHECK(bp.hash != hash_kind::none);
    CHECK((int)bp.sig >= 0 && (int)bp.sig <= 2 && (int)bp.key >= 0 && (int)bp.key <= 3);
    CHECK((bp.sig == sig_kind::msm) == pp.msm);
    CHECK((bp.key == key_kind::bits) == (s.src == key_source::bits));
    if (bp.key == key_kind::decompress) CHECK(s.src == key_source::bytes && bp.n_keys == s.keys_per_set * n);
    if (bp.key == key_kind::table) CHECK(s.src == key_source::table);
    if (s.src != key_source::bytes) CHECK(bp.n_keys == 0);
  } else
    CHECK(bp.hash == hash_kind::none);
  CHECK(pp.split != pp.wave && (bp.line_group != 0) == pp.split);
  CHECK(!bp.late_join || (pp.msm && pp.split));
  // pairs
  CHECK(pp.per >= 1 && TB_LINE_CHUNK % pp.per == 0);
  CHECK(pp.n_f() == pp.nseg * pp.n_groups() + pp.n_xwave);
  CHECK(pp.n_main + pp.n_xwave == pp.n_pairs && (uint64_t)pp.n_groups() * pp.per >= pp.n_main);
  // product levels: each output fits its region, scratch levels alternate
  // fpart / fpart2, each level reads what the one before wrote, the last
  // writes the partial (or segv, followed by the combine)
  if (settle) {
    CHECK(bp.n_levels == 0 && !bp.combine);
    return;
  }
  CHECK(bp.n_levels >= 1 && bp.n_levels <= (int)(sizeof(bp.levels) / sizeof(bp.levels[0])));
  CHECK(bp.combine == (pp.seg() && pp.nseg > 1));
  const uint32_t rows = bp.combine ? pp.nseg : 1;
  for (int i = 0; i < bp.n_levels; i++) {
    const prod_level& l = bp.levels[i];
    const bool last = i + 1 == bp.n_levels;
    CHECK(l.seg == bp.combine);
    CHECK(l.n_out == (l.n_in_last + l.chunk - 1) / l.chunk && l.n_in <= l.n_in_last);
    if (last) {
      CHECK(l.n_out == 1 && l.dst == (bp.combine ? prod_dst::segv : prod_dst::partial));
    } else {
      CHECK(l.n_out > 1 && l.dst == ((i & 1) ? prod_dst::fpart2 : prod_dst::fpart));
      const size_t room = (i & 1) ? L.segv - L.fpart2 : L.fpart2 - L.fpart;
      CHECK((size_t)rows * l.n_out * sizeof(tb::fp12) <= room);
    }
    if (l.seg) {
      CHECK(l.out_stride == (last ? 1u : l.n_out));
      CHECK((uint64_t)(rows - 1) * l.in_stride + l.n_in_last <= (i ? (uint64_t)rows * bp.levels[i - 1].n_out : (uint64_t)pp.n_f()));
      if (i) CHECK(l.in_stride == bp.levels[i - 1].out_stride && l.n_in_last == bp.levels[i - 1].n_out);
    } else if (i)
      CHECK(l.n_in == bp.levels[i - 1].n_out);
    else
      CHECK(l.n_in == (pp.n_f() ? pp.n_f() : 1u));
  }
}

// The settle scratch (settle_layout) at n sets: regions 256-byte aligned, in
// order (each ends where the next begins, so disjoint), each large enough for
// nseg rows of its count of Fp12 values, or n words / n bytes.
static void check_settle(uint32_t n) {
  g_where = "settle_layout n=" + std::to_string(n);
  const settle_layout S(n);
  const size_t off[] = {S.V, S.A, S.B, S.list, S.out, S.total};
  CHECK(off[0] == 0);
  for (size_t o : off) CHECK(o % 256 == 0);
  for (int i = 0; i + 1 < 6; i++) CHECK(off[i] <= off[i + 1]);
  CHECK(S.nseg == settle_nseg(n) && S.nseg >= 1 && S.nseg <= 16);
  CHECK((uint64_t)S.nA * TB_SETTLE_FAN >= n && (uint64_t)S.nB * TB_SETTLE_FAN >= S.nA);  // every set in a group, every group in one above
  CHECK((n == 0 || ((uint64_t)S.nA - 1) * TB_SETTLE_FAN < n) && (S.nA == 0 || ((uint64_t)S.nB - 1) * TB_SETTLE_FAN < S.nA));
  CHECK(S.A - S.V >= (size_t)S.nseg * n * sizeof(tb::fp12));
  CHECK(S.B - S.A >= (size_t)S.nseg * S.nA * sizeof(tb::fp12));
  CHECK(S.list - S.B >= (size_t)S.nseg * S.nB * sizeof(tb::fp12));
  CHECK(S.out - S.list >= (size_t)n * 4);  // a test list is at most the n sets (nA, nB <= n)
  CHECK(S.total - S.out >= n);
  CHECK(S.nA <= n && S.nB <= std::max(n, 1u));
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "dump")) {
    sweep(plan_env::get(), dump);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "check")) {
    struct named_env {
      std::string name;
      plan_env env;
    };
    std::vector<named_env> envs;
    envs.push_back({"default", plan_env()});
    for (const char* a : {"0", "8,4", "1,2", "4,1", "2,3", "8,2", "16,16", "16,5", "2,16", "4,3"}) {  // tests/test_gpu_accseg.py
      plan_env e;
      e.parse_acc_plan(a);
      envs.push_back({std::string("TBLS_ACC_PLAN=") + a, e});
    }
    plan_env e;
    e.parse_w2("0");
    envs.push_back({"TBLS_W2=0", e});
    e = plan_env();
    e.parse_coop("0");
    envs.push_back({"TBLS_COOP=0", e});
    e = plan_env();
    e.parse_hash_plan("0,0,0");
    envs.push_back({"TBLS_HASH_PLAN=0,0,0", e});
    e = plan_env();
    e.parse_miller_wave_max("40000");
    envs.push_back({"TBLS_MILLER_WAVE_MAX=40000", e});
    e.parse_msm_min("40000");
    envs.push_back({"TBLS_MILLER_WAVE_MAX=40000 TBLS_MSM_MIN=40000", e});
    unsigned plans = 0;
    for (const named_env& ne : envs)
      sweep(ne.env, [&](uint32_t n, const source& s, bool settle, const batch_plan& bp) {
        check(n, s, settle, bp, ne.name.c_str());
        plans++;
      });
    for (uint32_t n : SIZES)
      if (n <= TB_SETTLE_MAX) check_settle(n);
    printf("plans %u failures %d\n", plans, g_fail);
    return g_fail ? 1 : 0;
  }
  fprintf(stderr, "usage: plan_check dump|check\n");
  return 2;
}
