// CPU check of the learned key cache's index functions
// (teku_amd/csrc/tb_pkindex.h pkx_cache, pkx_append, pkx_find_two;
// tests/test_pkcache_check.py): the append and the two-level lookup that the
// device runs (k_pk_learn, k_pk_lookup), on the host at 8 rows / 16 slots.
// Built with AddressSanitizer + UndefinedBehaviorSanitizer and run directly;
// the wrapper also builds it with -DTB_PKX_PROBE_MAX=3, a bound below the row
// count.  Prints "failures 0" when every case holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "tb_pkindex.h"

using namespace tb;

static int failures = 0;
#define CHECK(c)                                         \
  do {                                                   \
    if (!(c)) {                                          \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      failures++;                                        \
    }                                                    \
  } while (0)

static const uint32_t ROWS = 8, SLOTS = 16, MASK = SLOTS - 1;
static const uint64_t SEED = 0x0123456789abcdefull, TAB_SEED = 0xfedcba9876543210ull;

struct key48 {
  uint8_t b[48];
};

static key48 make_key(uint32_t ctr) {
  key48 k;
  for (int i = 0; i < 48; i++) k.b[i] = (uint8_t)(0x11 * i + 7);
  k.b[0] = 0x80 | (k.b[0] & 0x1f);
  memcpy(k.b + 20, &ctr, 4);
  return k;
}

static void words(uint32_t w[TB_PKX_WORDS], const key48& k) { memcpy(w, k.b, 48); }

// the point a key stands for here: 24 words that spell out the key's counter
static void point_of(uint32_t pt[TB_PKX_POINT_WORDS], const key48& k) {
  uint32_t ctr;
  memcpy(&ctr, k.b + 20, 4);
  for (uint32_t i = 0; i < TB_PKX_POINT_WORDS; i++) pt[i] = ctr * 131u + i + ((uint32_t)k.b[0] << 24) + ((uint32_t)k.b[47] << 8);
}

static uint32_t first_slot(const key48& k) {
  uint32_t w[TB_PKX_WORDS];
  words(w, k);
  return pkx_first(pkx_hash(w, SEED), MASK);
}

static std::vector<key48> keys_at(uint32_t slot, size_t count, uint32_t* ctr) {
  std::vector<key48> out;
  while (out.size() < count) {
    const key48 k = make_key((*ctr)++);
    if (first_slot(k) == slot) out.push_back(k);
  }
  return out;
}

// a cache of exactly ROWS rows and SLOTS slots: every array at its exact size,
// so an index past a row or a slot is an AddressSanitizer report
struct cache {
  std::vector<uint32_t> slots, keys, points;
  uint32_t n_rows = 0;
  unsigned long long stat[TB_PKC_STATS] = {0, 0, 0};
  cache() : slots(SLOTS, 0), keys(ROWS * TB_PKX_WORDS, 0xdeadbeefu), points(ROWS * TB_PKX_POINT_WORDS, 0xdeadbeefu) {}
  pkx_cache view() { return {slots.data(), MASK, keys.data(), points.data(), ROWS, &n_rows, stat, SEED}; }
  uint32_t add(const key48& k) {
    uint32_t w[TB_PKX_WORDS], pt[TB_PKX_POINT_WORDS];
    words(w, k);
    point_of(pt, k);
    return pkx_append(view(), w, pt);
  }
  uint32_t find(const key48& k) {
    uint32_t w[TB_PKX_WORDS];
    words(w, k);
    return pkx_find(slots.data(), MASK, keys.data(), w, SEED);
  }
  // found, and the row holds the key's bytes and its point
  bool holds(const key48& k) {
    const uint32_t r = find(k);
    if (r == TB_PKX_MISS || r >= ROWS) return false;
    uint32_t pt[TB_PKX_POINT_WORDS];
    point_of(pt, k);
    return memcmp(keys.data() + (size_t)r * TB_PKX_WORDS, k.b, 48) == 0 && memcmp(points.data() + (size_t)r * TB_PKX_POINT_WORDS, pt, sizeof pt) == 0;
  }
  uint32_t used() const {
    uint32_t n = 0;
    for (uint32_t s : slots) n += s != 0;
    return n;
  }
};

int main() {
  const uint32_t B = pkx_probe_bound(SLOTS);
  CHECK(B == (TB_PKX_PROBE_MAX < SLOTS ? TB_PKX_PROBE_MAX : SLOTS));
  CHECK(pkx_capacity(ROWS) == SLOTS);  // the load factor stays at most 1/2
  uint32_t ctr = 0;

  {  // insert then find
    cache c;
    const key48 a = make_key(ctr++), b = make_key(ctr++), x = make_key(ctr++);
    CHECK(c.find(a) == TB_PKX_MISS);
    CHECK(c.add(a) == 0 && c.add(b) == 1);
    CHECK(c.holds(a) && c.holds(b) && c.find(a) == 0 && c.find(b) == 1 && c.find(x) == TB_PKX_MISS);
    CHECK(c.n_rows == 2 && c.used() == 2 && c.stat[TB_PKC_LEARNED] == 2 && c.stat[TB_PKC_REFUSED] == 0 && c.stat[TB_PKC_HITS] == 0);
  }

  {  // the same bytes twice: one findable entry, no second row, no second slot
    cache c;
    const key48 a = make_key(ctr++), b = make_key(ctr++);
    CHECK(c.add(a) == 0);
    CHECK(c.add(a) == TB_PKX_DUP);
    CHECK(c.add(b) == 1);
    CHECK(c.add(a) == TB_PKX_DUP && c.add(b) == TB_PKX_DUP);
    CHECK(c.n_rows == 2 && c.used() == 2 && c.stat[TB_PKC_LEARNED] == 2);
    CHECK(c.holds(a) && c.holds(b));
  }

  {  // neighbours: a flag bit of the first byte, the last byte
    const key48 a = make_key(ctr++);
    key48 f = a, s = a, l = a;
    f.b[0] ^= 0x20;
    s.b[0] ^= 0x40;
    l.b[47] ^= 0x01;
    {
      cache c;
      CHECK(c.add(a) == 0);
      CHECK(c.holds(a) && c.find(f) == TB_PKX_MISS && c.find(s) == TB_PKX_MISS && c.find(l) == TB_PKX_MISS);
    }
    {
      cache c;
      CHECK(c.add(a) == 0 && c.add(f) == 1 && c.add(l) == 2 && c.add(s) == 3);
      CHECK(c.holds(a) && c.holds(f) && c.holds(l) && c.holds(s) && c.used() == 4);
      CHECK(c.find(a) == 0 && c.find(f) == 1 && c.find(l) == 2 && c.find(s) == 3);
    }
  }

  {  // a probe chain that wraps past the last slot
    cache c;
    const std::vector<key48> k = keys_at(MASK, 4, &ctr);
    CHECK(c.add(k[0]) == 0 && c.add(k[1]) == 1 && c.add(k[2]) == 2);
    CHECK(c.slots[MASK] == 1 && c.slots[0] == 2 && c.slots[1] == 3 && c.used() == 3);
    for (int i = 0; i < 3; i++) CHECK(c.holds(k[i]));
    CHECK(c.find(k[3]) == TB_PKX_MISS);
    CHECK(c.add(k[1]) == TB_PKX_DUP);  // found behind the wrap
  }

  if (B < ROWS) {  // the probe bound: the next key of a full chain is not appended, takes no row, and is not found
    cache c;
    const uint32_t s0 = 14;
    const std::vector<key48> k = keys_at(s0, B + 1, &ctr);
    for (uint32_t i = 0; i < B; i++) CHECK(c.add(k[i]) == i);
    const std::vector<uint32_t> before = c.slots;
    CHECK(c.add(k[B]) == TB_PKX_MISS);
    CHECK(before == c.slots && c.n_rows == B && c.stat[TB_PKC_LEARNED] == B && c.stat[TB_PKC_REFUSED] == 0);
    CHECK(c.find(k[B]) == TB_PKX_MISS);
    for (uint32_t i = 0; i < B; i++) CHECK(c.holds(k[i]));
    const std::vector<key48> e = keys_at((s0 + B) & MASK, 1, &ctr);  // a key that starts where the chain ends still goes in
    CHECK(c.add(e[0]) == B && c.holds(e[0]));
  }

  {  // a full cache refuses, counts the refusal, and still finds what it holds
    cache c;
    std::vector<key48> k;
    std::vector<bool> went;
    uint32_t in = 0;
    unsigned long long refused = 0;
    while (in < ROWS && k.size() < 64) {  // fill every row
      k.push_back(make_key(ctr++));
      const uint32_t r = c.add(k.back());
      went.push_back(r < ROWS);
      if (r < ROWS) {
        CHECK(r == in);
        in++;
      } else {
        CHECK(r == TB_PKX_MISS && B < SLOTS);  // no slot within the bound: the short-bound build only
      }
    }
    CHECK(in == ROWS && c.n_rows == ROWS && c.used() == ROWS && c.stat[TB_PKC_REFUSED] == 0);
    for (int i = 0; i < 3; i++) {  // three more keys: refused where the probe reaches a free slot
      k.push_back(make_key(ctr++));
      went.push_back(false);
      const uint32_t r = c.add(k.back());
      CHECK(r == TB_PKX_FULL || (r == TB_PKX_MISS && B < SLOTS));
      refused += r == TB_PKX_FULL;
    }
    CHECK(c.stat[TB_PKC_LEARNED] == ROWS && c.stat[TB_PKC_REFUSED] == refused && (refused == 3 || B < SLOTS));
    CHECK(c.n_rows == ROWS && c.used() == ROWS);
    for (size_t i = 0; i < k.size(); i++) CHECK(went[i] ? c.holds(k[i]) : c.find(k[i]) == TB_PKX_MISS);
    for (size_t i = 0; i < k.size(); i++)
      if (went[i]) CHECK(c.add(k[i]) == TB_PKX_DUP);  // a held key is no refusal
    CHECK(c.stat[TB_PKC_REFUSED] == refused && c.n_rows == ROWS);
    CHECK(c.add(make_key(ctr++)) != TB_PKX_DUP && c.n_rows == ROWS && c.used() == ROWS);
  }

  {  // the two-level lookup: the table first, then the cache
    std::vector<uint32_t> tkeys;
    uint32_t tslots[8];
    memset(tslots, 0, sizeof tslots);
    const key48 both = make_key(ctr++), only_tab = make_key(ctr++), only_cache = make_key(ctr++), none = make_key(ctr++);
    for (const key48* k : {&both, &only_tab}) {
      tkeys.resize(tkeys.size() + TB_PKX_WORDS);
      memcpy(tkeys.data() + tkeys.size() - TB_PKX_WORDS, k->b, 48);
      CHECK(pkx_insert(tslots, 7u, tkeys.data(), (uint32_t)(tkeys.size() / TB_PKX_WORDS - 1), TAB_SEED) != TB_PKX_MISS);
    }
    cache c;
    CHECK(c.add(only_cache) == 0 && c.add(both) == 1);
    const pkx_cache cv = c.view(), no_cache = {nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0};
    const auto look = [&](const uint32_t* ts, const pkx_cache& cc, const key48& k) {
      uint32_t w[TB_PKX_WORDS];
      words(w, k);
      return pkx_find_two(ts, 7u, tkeys.data(), TAB_SEED, cc, w);
    };
    pkx_hit h = look(tslots, cv, both);
    CHECK(h.src == TB_PKX_SRC_TABLE && h.idx == 0);
    h = look(tslots, cv, only_tab);
    CHECK(h.src == TB_PKX_SRC_TABLE && h.idx == 1);
    h = look(tslots, cv, only_cache);
    CHECK(h.src == TB_PKX_SRC_CACHE && h.idx == 0);
    h = look(tslots, cv, none);
    CHECK(h.src == TB_PKX_SRC_NONE && h.idx == TB_PKX_MISS);
    // no table: the cache alone; no cache: the table alone; neither: a miss
    h = look(nullptr, cv, both);
    CHECK(h.src == TB_PKX_SRC_CACHE && h.idx == 1);
    h = look(nullptr, cv, only_tab);
    CHECK(h.src == TB_PKX_SRC_NONE);
    h = look(tslots, no_cache, only_cache);
    CHECK(h.src == TB_PKX_SRC_NONE);
    h = look(tslots, no_cache, both);
    CHECK(h.src == TB_PKX_SRC_TABLE && h.idx == 0);
    h = look(nullptr, no_cache, both);
    CHECK(h.src == TB_PKX_SRC_NONE && h.idx == TB_PKX_MISS);
  }

  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
