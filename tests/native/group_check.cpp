// CPU check of the message grouping and the grouped staging image
// (teku_amd/csrc/tb_group.h; tests/test_group_host.py).  For each case:
// group_messages, pack_layout_grouped, then pack_fill_grouped into a heap
// block of exactly `total` bytes pre-filled with the marker byte 0xA5 (so ASan
// sees a write past the image), then one line
//   case <name> n=<n> m=<m> K=<K> M=<M> set_grp=<n ids> off=<the nine region offsets> total=<total> image=<hex>
// (a list of no entries prints as "-").  The sets' keys, signatures and
// randomizers are the byte patterns of pack_check.cpp; the messages are
// spelled out per case, and tests/test_group_host.py spells out the same.
#include <cstdio>
#include <string>
#include <vector>

#include "tb_group.h"

using namespace tb::group;

static const uint8_t MARK = 0xA5;

static uint8_t pat(uint32_t tag, uint32_t i, uint32_t j) { return (uint8_t)(tag * 61u + i * 17u + j * 7u + 3u); }

struct msg_ref {
  const uint8_t* p;
  uint32_t len;
};

// n = msgs.size() sets of one 48-byte key each; set i signs msgs[i]
static void emit(const char* name, const std::vector<msg_ref>& msgs, size_t lo, size_t hi, bool with_rand, uint32_t dlen) {
  const uint32_t n = (uint32_t)msgs.size();
  std::vector<std::vector<uint8_t>> keys(n, std::vector<uint8_t>(48)), sigs(n, std::vector<uint8_t>(96));
  std::vector<uint64_t> rand(n);
  std::vector<uint8_t> dst(dlen);
  std::vector<tbls_set> sets;
  for (uint32_t i = 0; i < n; i++) {
    for (uint32_t j = 0; j < 48; j++) keys[i][j] = pat(1, i, j);
    for (uint32_t j = 0; j < 96; j++) sigs[i][j] = pat(3, i, j);
    rand[i] = 0x0102030405060708ull * (i + 1) + i;
    sets.push_back({keys[i].data(), 1, msgs[i].p, msgs[i].len, sigs[i].data()});
  }
  for (uint32_t j = 0; j < dlen; j++) dst[j] = pat(4, 0, j);
  const groups G = group_messages(sets.data(), lo, hi);
  const packed_grouped p = pack_layout_grouped(sets.data(), lo, hi, dlen, G);
  uint8_t* h = new uint8_t[p.total];
  memset(h, MARK, p.total);
  pack_fill_grouped(h, p, sets.data(), lo, with_rand ? rand.data() : nullptr, dlen ? dst.data() : nullptr, dlen, G);
  printf("case %s n=%u m=%u K=%u M=%u set_grp=", name, p.n, p.m, p.K, p.M);
  if (G.set_grp.empty()) printf("-");
  for (size_t i = 0; i < G.set_grp.size(); i++) printf("%s%u", i ? "," : "", G.set_grp[i]);
  printf(" off=%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu total=%zu image=", p.off_pks, p.off_pkoff, p.off_msgs, p.off_msgoff, p.off_sigs, p.off_rand,
         p.off_dst, p.off_grpoff, p.off_grpsets, p.total);
  for (size_t i = 0; i < p.total; i++) printf("%02x", h[i]);
  printf("\n");
  delete[] h;
}

// a heap copy of exactly len bytes, so ASan sees a read past a message
static uint8_t* heap(const std::string& s) {
  uint8_t* p = new uint8_t[s.size() ? s.size() : 1];
  memcpy(p, s.data(), s.size());
  return p;
}

int main() {
  emit("empty", {}, 0, 0, false, 43);
  {  // every message distinct
    uint8_t *a = heap("alpha"), *b = heap("beta"), *c = heap("gamma!");
    emit("distinct", {{a, 5}, {b, 4}, {c, 6}}, 0, 3, true, 43);
    delete[] a, delete[] b, delete[] c;
  }
  {  // every message equal: one pointer, and equal bytes at three addresses
    uint8_t *a = heap("same-root"), *b = heap("same-root"), *c = heap("same-root");
    emit("equal_ptr", {{a, 9}, {a, 9}, {a, 9}, {a, 9}}, 0, 4, false, 43);
    emit("equal_bytes", {{a, 9}, {b, 9}, {c, 9}}, 0, 3, true, 0);
    delete[] a, delete[] b, delete[] c;
  }
  {  // one address with different lengths; a message that is a prefix of another; interleaved groups
    uint8_t *a = heap("abcdefgh"), *b = heap("abcd");
    emit("same_ptr_lens", {{a, 8}, {a, 4}, {a, 8}, {b, 4}, {a, 0}}, 0, 5, true, 43);
    delete[] a, delete[] b;
  }
  {  // zero-length messages: a null pointer and a real one are the same message
    uint8_t *a = heap(""), *b = heap("x");
    emit("zero_len", {{nullptr, 0}, {b, 1}, {a, 0}, {nullptr, 0}}, 0, 4, false, 43);
    emit("all_zero_len", {{nullptr, 0}, {a, 0}}, 0, 2, false, 43);
    delete[] a, delete[] b;
  }
  {  // the sub-range [1, 3) of four sets, rebased: sets 0 and 3 play no part
    uint8_t *a = heap("outside"), *b = heap("inner"), *c = heap("inner");
    emit("range_1_3", {{a, 7}, {b, 5}, {c, 5}, {a, 7}}, 1, 3, true, 43);
    delete[] a, delete[] b, delete[] c;
  }
  return 0;
}
