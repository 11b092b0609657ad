// CPU check of the batch plan and the staging image with the hash-point memo
// (teku_amd/csrc/tb_plan.h batch_plan::n_hash, ws_layout::Qh / skiph;
// tb_msgmemo.h pack_layout_memo / pack_fill_memo; tests/test_memo_plan.py).
// Prints one line per failed check and `ok <count>` when none failed.
#include <cstdio>
#include <string>
#include <vector>

#include "tb_msgmemo.h"

using namespace tb::plan;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    g_checks++;                               \
    if (!(cond)) {                            \
      g_failed++;                             \
      printf("FAIL %s:%d: ", #cond, __LINE__); \
      printf(__VA_ARGS__);                    \
      printf("\n");                           \
    }                                         \
  } while (0)

// every offset of a layout, in declaration order
static std::vector<size_t> offsets(const ws_layout& L) {
  return {L.pk_aff, L.pk_code, L.P, L.Q, L.skip, L.set_code, L.sig_code, L.f, L.fpart, L.fpart2, L.segv, L.n_bad, L.result, L.sig_aff,
          L.sig_use, L.msm_cnt, L.msm_off, L.msm_cur, L.msm_idx, L.msm_sum, L.mlist, L.mcnt, L.lines, L.hrow, L.pair_code, L.set_P,
          L.grp_item, L.grp_part, L.grp_pskip, L.code_bytes};
}

int main() {
  const plan_env env;  // the defaults, whatever the environment says
  const uint32_t sizes[] = {8, 600, 2304, 16384};
  // 1. memo off: the plan and every offset are what they are with the new
  // parameter left at its default, Qh / skiph are empty and last
  for (uint32_t n : sizes)
    for (int settle = 0; settle < 2; settle++)
      for (uint32_t n_msgs : {0u, n / 4}) {
        const batch_plan a(n, n, key_source::bytes, settle != 0, env, n_msgs), b(n, n, key_source::bytes, settle != 0, env, n_msgs, HASH_ALL);
        const ws_layout A(a), B(b);
        CHECK(!a.memo && a.n_hash == a.pp.n_msgs && a.hash == b.hash, "n=%u", n);
        CHECK(offsets(A) == offsets(B) && A.total == B.total, "n=%u", n);
        CHECK(A.Qh == A.skiph && A.skiph == A.total, "n=%u: Qh %zu skiph %zu total %zu", n, A.Qh, A.skiph, A.total);
        // and a memo plan that hashes everything moves nothing either: it only appends
        const batch_plan m(n, n, key_source::bytes, settle != 0, env, n_msgs, a.pp.n_msgs);
        const ws_layout M(m);
        CHECK(m.memo && m.hash == a.hash && offsets(M) == offsets(A), "n=%u", n);
      }
  // 2. memo on: Qh / skiph hold n_hash entries behind every other region, 16-byte aligned
  for (uint32_t n : sizes)
    for (uint32_t mh : {0u, 1u, 3u, n / 2, n}) {
      const batch_plan bp(n, n, key_source::bytes, false, env, 0, mh);
      const ws_layout L(bp);
      CHECK(bp.memo && bp.n_hash == mh && bp.pp.n_msgs == n, "n=%u mh=%u", n, mh);
      size_t end = 0;
      for (size_t o : offsets(L))
        if (o != L.code_bytes) end = std::max(end, o);
      CHECK(L.Qh >= end && L.Qh >= L.grp_pskip, "n=%u mh=%u", n, mh);
      CHECK(L.Qh % 16 == 0 && L.Q % 16 == 0 && L.skiph >= L.Qh + (size_t)mh * sizeof(tb::g2a) && L.total >= L.skiph + mh, "n=%u mh=%u", n, mh);
      CHECK(L.hrow + (bp.hash == hash_kind::row ? (size_t)mh * HROW_SET_BYTES : 0) <= L.lines, "n=%u mh=%u", n, mh);
    }
  // 3. the hash kernel follows the messages to hash
  CHECK(batch_plan(16384, 16384, key_source::bytes, false, env, 0, 3).hash == hash_kind::coop, "16,384 sets, 3 to hash");
  CHECK(batch_plan(16384, 16384, key_source::bytes, false, env, 0, 0).hash == hash_kind::none, "16,384 sets, none to hash");
  CHECK(batch_plan(16384, 16384, key_source::bytes, false, env, 0, 600).hash == hash_kind::row, "16,384 sets, 600 to hash");
  CHECK(batch_plan(16384, 16384, key_source::bytes, false, env, 0, 16384).hash == hash_kind::duo, "16,384 sets, all to hash");
  CHECK(batch_plan(16384, 16384, key_source::bytes, false, env).hash == hash_kind::duo, "16,384 sets, no memo");
  CHECK(batch_plan(16384, 16384, key_source::bytes, false, env, 64, 2).hash == hash_kind::coop, "grouped, 2 of 64 to hash");
  CHECK(batch_plan(128, 128, key_source::bytes, false, env, 0, 0).hash == hash_kind::none, "128 sets, none to hash");
  // 4. the w2 kernel's park area (a g2a per hashed message) fits the line buffer, split plan or not
  {
    const batch_plan bp(65536, 65536, key_source::bytes, false, env, 0, 40000);
    const ws_layout L(bp);
    CHECK(bp.hash == hash_kind::w2, "65,536 sets, 40,000 to hash: kind %d", (int)bp.hash);
    CHECK(L.f - L.lines >= (size_t)40000 * sizeof(tb::g2a), "park area %zu", L.f - L.lines);
    plan_env wave = env;  // every pair on the wave Miller loops: no line buffer of its own
    wave.miller_wave_max = 1u << 20;
    wave.msm_min = 1u << 30;
    const batch_plan bw(65536, 65536, key_source::bytes, false, wave, 0, 40000);
    const ws_layout W(bw);
    CHECK(!bw.pp.split && bw.hash == hash_kind::w2 && W.f - W.lines >= (size_t)40000 * sizeof(tb::g2a), "unsplit: park area %zu", W.f - W.lines);
  }
  // 5. the image: the base regions where they were, the new ones behind them
  {
    std::vector<std::vector<uint8_t>> msgs = {{1, 2, 3}, {4, 5}, {1, 2, 3}, {}, {6}};
    std::vector<uint8_t> key(48, 7), sig(96, 9);
    std::vector<tbls_set> sets;
    for (auto& m : msgs) sets.push_back({key.data(), 1, m.empty() ? nullptr : m.data(), (uint32_t)m.size(), sig.data()});
    const tb::group::groups G = tb::group::group_messages(sets.data(), 0, sets.size());
    tb::memo::index X;
    X.configure(4);
    (void)X.resolve(sets.data(), 1, 2);  // {4, 5} resident in row 0
    for (int grouped = 0; grouped < 2; grouped++) {
      tb::memo::index Y = X;
      const tb::memo::resolved R = Y.resolve(G, !grouped);
      tb::group::packed_grouped base;
      if (grouped)
        base = tb::group::pack_layout_grouped(sets.data(), 0, sets.size(), 43, G);
      else
        static_cast<tb::pack::packed&>(base) = tb::pack::pack_layout(sets.data(), 0, sets.size(), 43);
      const tb::memo::packed_memo p = tb::memo::pack_layout_memo(base, grouped != 0, G, R);
      CHECK(p.off_pks == base.off_pks && p.off_pkoff == base.off_pkoff && p.off_msgs == base.off_msgs && p.off_msgoff == base.off_msgoff &&
                p.off_sigs == base.off_sigs && p.off_rand == base.off_rand && p.off_dst == base.off_dst,
            "grouped=%d", grouped);
      if (grouped) CHECK(p.off_grpoff == base.off_grpoff && p.off_grpsets == base.off_grpsets, "the CSR moved");
      CHECK(p.off_hmsgs == base.total && p.off_hmsgoff == p.off_hmsgs + 256 && p.off_src == p.off_hmsgoff + 256 && p.off_learn == p.off_src + 256 &&
                p.off_setgrp == p.off_learn + 256 && p.total == p.off_setgrp + (grouped ? 0 : 256),
            "grouped=%d", grouped);
      CHECK(p.m_hash == 3 && p.HM == 4 && p.groups == 4, "m_hash %u HM %u groups %u", p.m_hash, p.HM, p.groups);
      std::vector<uint8_t> img(p.total, 0xA5);  // exactly total bytes: ASan sees a write past the image
      tb::memo::pack_fill_memo(img.data(), p, G, R);
      const uint32_t *off = (const uint32_t*)(img.data() + p.off_hmsgoff), *src = (const uint32_t*)(img.data() + p.off_src),
                     *learn = (const uint32_t*)(img.data() + p.off_learn);
      CHECK(off[0] == 0 && off[1] == 3 && off[2] == 3 && off[3] == 4, "offsets");
      CHECK(img[p.off_hmsgs] == 1 && img[p.off_hmsgs + 2] == 3 && img[p.off_hmsgs + 3] == 6 && img[p.off_hmsgs + 4] == 0xA5, "bytes");
      CHECK(src[0] == 0 && src[1] == (tb::memo::SRC_ROW | 0u) && src[2] == 1 && src[3] == 2, "src");
      CHECK(learn[0] == 1 && learn[1] == 2 && learn[2] == 3, "learn");
      if (!grouped) {
        const uint32_t* sg = (const uint32_t*)(img.data() + p.off_setgrp);
        CHECK(sg[0] == 0 && sg[1] == 1 && sg[2] == 0 && sg[3] == 2 && sg[4] == 3, "set_grp");
      }
      for (size_t i = 0; i < base.total; i++)
        if (img[i] != 0xA5) {
          CHECK(false, "pack_fill_memo wrote into the base image at %zu", i);
          break;
        }
    }
  }
  if (!g_failed) printf("ok %d\n", g_checks);
  return g_failed ? 1 : 0;
}
