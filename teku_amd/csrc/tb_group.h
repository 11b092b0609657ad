// Grouping the sets of a host batch by message: sets[lo, hi) that sign the
// same bytes share one hash_to_G2 and one Miller loop ("Grouped
// batches"), so the grouped launch needs the distinct messages and, per
// distinct message, the list of its sets.  Plain host code, no HIP, and
// deterministic: tests/native/group_check.cpp compiles this header with g++
// and tests/test_group_host.py compares its output with the statement below.
// Not included by any kernel translation unit.
//
// Grouping.  Two messages are the same when their lengths and their bytes are
// equal (equal pointers with equal lengths only save the comparison).  Groups
// are numbered in the order in which their message first appears in
// sets[lo, hi).  The result, for n = hi - lo sets and m distinct messages:
//   m                 the number of groups (0 only when n is 0)
//   msg[g], len[g]    group g's message (the first appearance's pointer)
//   grp_off[m + 1]    grp_off[0] = 0, grp_off[m] = n
//   grp_sets[n]       group g's sets are grp_sets[grp_off[g] .. grp_off[g + 1]):
//                     set indices rebased to lo (set lo is 0), ascending
//                     inside a group
//   set_grp[n]        the group of set lo + i
//
// The staging image of a grouped launch has the regions of tb_pack.h, in the
// same order, followed by two more; each region starts at a multiple of 256
// bytes:
//   keys, key offsets, signatures, randomizers, DST
//                     exactly as in tb_pack.h (per set)
//   messages          the m distinct messages back to back, in group order
//                     (1 byte when all are empty)
//   msg offsets       m + 1 words, in bytes
//   CSR offsets       grp_off: m + 1 words (after the DST)
//   CSR sets          grp_sets: n words (1 word when n is 0)
// Bytes between a region's end and the next region are not written.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "tb_pack.h"

namespace tb {
namespace group {

using pack::packed;
using plan::align_up;

struct groups {
  uint32_t m = 0;
  uint64_t M = 0;  // bytes of the distinct messages
  std::vector<const uint8_t*> msg;
  std::vector<uint32_t> len, grp_off, grp_sets, set_grp;
};

// FNV-1a over the bytes, the length mixed in
inline uint64_t msg_hash(const uint8_t* p, uint32_t len) {
  uint64_t h = 0xcbf29ce484222325ull ^ len;
  for (uint32_t i = 0; i < len; i++) h = (h ^ p[i]) * 0x100000001b3ull;
  return h ^ (h >> 29);
}

template <class SET>
groups group_messages(const SET* sets, size_t lo, size_t hi) {
  groups G;
  const uint32_t n = (uint32_t)(hi - lo);
  G.set_grp.resize(n);
  G.grp_off.assign(1, 0u);
  if (!n) return G;
  // open addressing over group ids (slot value g + 1; 0: free)
  size_t cap = 16;
  while (cap < 2 * (size_t)n) cap *= 2;
  std::vector<uint32_t> slot(cap, 0u);
  std::vector<uint32_t> count;
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t* p = sets[lo + i].msg;
    const uint32_t len = sets[lo + i].msg_len;
    size_t s = (size_t)msg_hash(p, len) & (cap - 1);
    uint32_t g;
    for (;;) {
      if (!slot[s]) {
        g = G.m++;
        slot[s] = g + 1;
        G.msg.push_back(p);
        G.len.push_back(len);
        G.M += len;
        count.push_back(0u);
        break;
      }
      g = slot[s] - 1;
      if (G.len[g] == len && (G.msg[g] == p || !len || !memcmp(G.msg[g], p, len))) break;
      s = (s + 1) & (cap - 1);
    }
    G.set_grp[i] = g;
    count[g]++;
  }
  G.grp_off.resize((size_t)G.m + 1);
  for (uint32_t g = 0; g < G.m; g++) G.grp_off[g + 1] = G.grp_off[g] + count[g];
  G.grp_sets.resize(n);
  std::vector<uint32_t> cur(G.grp_off.begin(), G.grp_off.end() - 1);
  for (uint32_t i = 0; i < n; i++) G.grp_sets[cur[G.set_grp[i]]++] = i;  // ascending i: ascending inside a group
  return G;
}

// the image's layout: tb_pack.h's, the message regions sized by the distinct
// messages, then the CSR
struct packed_grouped : packed {
  size_t off_grpoff, off_grpsets;
  uint32_t m;
};

template <class SET>
packed_grouped pack_layout_grouped(const SET* sets, size_t lo, size_t hi, uint32_t dlen, const groups& G) {
  packed_grouped p;
  p.n = (uint32_t)(hi - lo);
  p.m = G.m;
  uint64_t K = 0;
  for (size_t i = lo; i < hi; i++) K += sets[i].n_pks;
  p.K = (uint32_t)K;
  p.M = (uint32_t)G.M;
  size_t o = 0;
  p.off_pks = o;     o = align_up(o + (size_t)K * pack::key_bytes<SET>());
  p.off_pkoff = o;   o = align_up(o + ((size_t)p.n + 1) * 4);
  p.off_msgs = o;    o = align_up(o + (p.M ? p.M : 1));
  p.off_msgoff = o;  o = align_up(o + ((size_t)p.m + 1) * 4);
  p.off_sigs = o;    o = align_up(o + (size_t)p.n * 96);
  p.off_rand = o;    o = align_up(o + (size_t)p.n * 8);
  p.off_dst = o;     o = align_up(o + (dlen ? dlen : 1));
  p.off_grpoff = o;  o = align_up(o + ((size_t)p.m + 1) * 4);
  p.off_grpsets = o; o = align_up(o + (p.n ? (size_t)p.n * 4 : 4));
  p.total = o;
  return p;
}

// the image of sets[lo, lo + p.n) with the groups G at h (p.total bytes); rand (nullable) is indexed like sets
template <class SET>
void pack_fill_grouped(uint8_t* h, const packed_grouped& p, const SET* sets, size_t lo, const uint64_t* rand, const uint8_t* dst,
                       uint32_t dlen, const groups& G) {
  uint32_t* pkoff = (uint32_t*)(h + p.off_pkoff);
  uint32_t* moff = (uint32_t*)(h + p.off_msgoff);
  uint64_t* rr = (uint64_t*)(h + p.off_rand);
  uint32_t k = 0, mb = 0;
  for (uint32_t i = 0; i < p.n; i++) {
    const SET& s = sets[lo + i];
    pkoff[i] = k;
    pack::pack_keys(h + p.off_pks + (size_t)k * pack::key_bytes<SET>(), s);
    memcpy(h + p.off_sigs + (size_t)i * 96, s.sig, 96);
    rr[i] = rand ? rand[lo + i] : 1;
    k += s.n_pks;
  }
  pkoff[p.n] = k;
  for (uint32_t g = 0; g < p.m; g++) {
    moff[g] = mb;
    if (G.len[g]) memcpy(h + p.off_msgs + mb, G.msg[g], G.len[g]);
    mb += G.len[g];
  }
  moff[p.m] = mb;
  if (dlen) memcpy(h + p.off_dst, dst, dlen);
  memcpy(h + p.off_grpoff, G.grp_off.data(), ((size_t)p.m + 1) * 4);
  if (p.n) memcpy(h + p.off_grpsets, G.grp_sets.data(), (size_t)p.n * 4);
}

}  // namespace group
}  // namespace tb
