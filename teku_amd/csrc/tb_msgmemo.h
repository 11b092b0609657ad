// The hash-point memo's index: which message's H(m) each row of
// a device's resident row array holds.  H(m) depends on the message bytes and
// the batch entries' fixed DST alone, so a row written once serves every later
// batch that signs the same bytes.  The index lives on the host, inside the
// device context and under its lock, because only the host can know before
// launch how many messages are left to hash -- the count that picks the hash
// kernel and its grid (tb_plan.h batch_plan).  Plain host code, no HIP, and
// deterministic: tests/native/msgmemo_check.cpp compiles this header with g++
// and tests/test_msgmemo_host.py compares it with a dictionary model of the
// rules below.  Not included by any kernel translation unit.
//
// Rows.  R rows; row r holds one message of at most TB_MEMO_MSG_MAX bytes
// (longer messages are never resident; the empty message is cacheable).  Rows
// are handed out in order, 0, 1, 2, ...; none is ever freed alone.
//
// resolve.  Starts from the grouping of the shard's sets (tb_group.h: the
// distinct messages in first-appearance order).  Let `new` be the distinct
// cacheable messages that are not resident.
//   * new <= free rows: each takes the next free row, in first-appearance order;
//   * otherwise FLUSH: the whole index is emptied (and the flush counted),
//     every distinct cacheable message of the shard is new, the first
//     min(count, R) of them in first-appearance order take rows 0, 1, ..., and
//     the rest are hashed and not learned.
// The result, for m distinct messages:
//   m_hash[j]   the group whose message is the j-th to hash: the distinct
//               messages that were not resident plus the over-long ones, in
//               first-appearance order
//   src[g]      SRC_ROW | r: group g's point is row r's (learned by an earlier
//               call); else j: it is the j-th hashed message's
//   learn[j]    the row that hashed message j is stored into, or LEARN_NONE
// A resolve whose launch then fails must be followed by invalidate(): the
// device rows it promised may never have been written.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "tb_group.h"

#define TB_MEMO_MSG_MAX 64u
#define TB_MEMO_ROWS_MAX 1048576u
// Shards of more sets than this bypass the memo: they are staged and hashed as
// without one and leave the index as it is.  Resolving costs host time per
// set and per distinct message (grouping, the index, the image's extra
// regions) and a copy per pair on the device, which only repeated messages
// pay back.  Measured with tools/bench_msgmemo.py (profiles/msgmemo.json,
// tbls_batch_verify, memo off / memo on and cleared before each call): with
// every message distinct 16,384 sets 9.1-9.2 / 11.5 ms and 131,072 sets
// 36.1-36.3 / 46.7 ms, against memo-off spreads of 0.13 and 0.28 ms; with 64
// messages the warm memo wins at every size measured, 16,384 sets (8.84-8.89
// / 8.25 ms) being the largest -- and the largest batch the services form
// (DEFAULT_MAX_BATCH_SIZE).  So the cutoff is the largest size with a
// measured gain; above it nothing measured gains and the all-distinct cost is
// 29 %.  At and below it a service whose messages do not repeat still pays
// (2.3 ms at 16,384 distinct messages): the memo is opt-in for that reason.
#define TB_MEMO_SETS_MAX 16384u

namespace tb {
namespace memo {

constexpr uint32_t SRC_ROW = 0x80000000u;
constexpr uint32_t LEARN_NONE = 0xffffffffu;

struct resolved {
  std::vector<uint32_t> m_hash, src, learn;
  bool flushed = false;
};

struct index {
  uint32_t rows = 0, used = 0;
  uint64_t hits = 0, hashed = 0, flushes = 0;  // pairs served from a row, messages hashed, flushes
  std::vector<uint32_t> slot;                  // open addressing over rows (row + 1; 0: free), a power of two >= 2 rows
  std::vector<uint8_t> len, bytes;             // per row in use: the message's length and TB_MEMO_MSG_MAX bytes of it

  // rows per device (0: off); forgets everything learned, the counters too
  void configure(uint32_t r) {
    rows = r > TB_MEMO_ROWS_MAX ? TB_MEMO_ROWS_MAX : r;
    size_t cap = 16;
    while (cap < 2 * (size_t)rows) cap *= 2;
    slot.assign(rows ? cap : 0, 0u);
    len.clear();
    bytes.clear();
    used = 0;
    hits = hashed = flushes = 0;
  }
  void invalidate() {
    std::fill(slot.begin(), slot.end(), 0u);
    len.clear();
    bytes.clear();
    used = 0;
  }
  void reset_counters() { hits = hashed = flushes = 0; }

  // the row of message (p, n), or LEARN_NONE
  uint32_t find(const uint8_t* p, uint32_t n) const {
    if (!rows || n > TB_MEMO_MSG_MAX) return LEARN_NONE;
    const size_t mask = slot.size() - 1;
    for (size_t s = (size_t)group::msg_hash(p, n) & mask;; s = (s + 1) & mask) {
      if (!slot[s]) return LEARN_NONE;
      const uint32_t r = slot[s] - 1;
      if (len[r] == n && (!n || !memcmp(&bytes[(size_t)r * TB_MEMO_MSG_MAX], p, n))) return r;
    }
  }
  // message (p, n <= TB_MEMO_MSG_MAX), not resident, into the next free row (used < rows)
  uint32_t insert(const uint8_t* p, uint32_t n) {
    const uint32_t r = used++;
    len.push_back((uint8_t)n);
    bytes.resize((size_t)used * TB_MEMO_MSG_MAX);
    if (n) memcpy(&bytes[(size_t)r * TB_MEMO_MSG_MAX], p, n);
    const size_t mask = slot.size() - 1;
    size_t s = (size_t)group::msg_hash(p, n) & mask;
    while (slot[s]) s = (s + 1) & mask;
    slot[s] = r + 1;
    return r;
  }

  // per_set: the launch has one main pair per set (an ungrouped pass), so a
  // resident message serves as many pairs as it has sets; else one per group
  resolved resolve(const group::groups& G, bool per_set) {
    resolved R;
    R.src.resize(G.m);
    std::vector<uint32_t> row(G.m);
    uint32_t n_new = 0;
    for (uint32_t g = 0; g < G.m; g++) {
      row[g] = find(G.msg[g], G.len[g]);
      if (row[g] == LEARN_NONE && G.len[g] <= TB_MEMO_MSG_MAX) n_new++;
    }
    if (n_new > rows - used) {
      invalidate();
      flushes++;
      R.flushed = true;
      std::fill(row.begin(), row.end(), LEARN_NONE);
    }
    for (uint32_t g = 0; g < G.m; g++) {
      if (row[g] != LEARN_NONE) {
        R.src[g] = SRC_ROW | row[g];
        hits += per_set ? G.grp_off[g + 1] - G.grp_off[g] : 1u;
        continue;
      }
      R.src[g] = (uint32_t)R.m_hash.size();
      R.m_hash.push_back(g);
      R.learn.push_back(G.len[g] <= TB_MEMO_MSG_MAX && used < rows ? insert(G.msg[g], G.len[g]) : LEARN_NONE);
    }
    hashed += R.m_hash.size();
    return R;
  }
  template <class SET>
  resolved resolve(const SET* sets, size_t lo, size_t hi, bool per_set = true) {
    return resolve(group::group_messages(sets, lo, hi), per_set);
  }
};

// The staging image of a launch that resolved (tb_group.h packed_grouped, or
// tb_pack.h's regions with m = 0 when the pass is ungrouped): every region of
// the base image where it was, then, each at a multiple of 256 bytes,
//   hashed messages   the m_hash messages back to back (1 byte when all are empty)
//   hashed offsets    m_hash + 1 words, in bytes
//   src               one word per distinct message (1 word when there is none)
//   learn             one word per hashed message (1 word when there is none)
//   set_grp           an ungrouped pass only: the group of each set (n words)
// Bytes between a region's end and the next region are not written.
struct packed_memo : group::packed_grouped {
  size_t off_hmsgs, off_hmsgoff, off_src, off_learn, off_setgrp;
  uint32_t m_hash, HM, groups;  // hashed messages, their bytes, distinct messages
  bool has_setgrp;
};

inline packed_memo pack_layout_memo(const group::packed_grouped& base, bool grouped, const group::groups& G, const resolved& R) {
  packed_memo p;
  static_cast<group::packed_grouped&>(p) = base;
  p.m_hash = (uint32_t)R.m_hash.size();
  p.groups = G.m;
  p.has_setgrp = !grouped;
  uint64_t HM = 0;
  for (uint32_t g : R.m_hash) HM += G.len[g];
  p.HM = (uint32_t)HM;
  size_t o = base.total;
  using plan::align_up;
  p.off_hmsgs = o;   o = align_up(o + (HM ? HM : 1));
  p.off_hmsgoff = o; o = align_up(o + ((size_t)p.m_hash + 1) * 4);
  p.off_src = o;     o = align_up(o + (G.m ? (size_t)G.m * 4 : 4));
  p.off_learn = o;   o = align_up(o + (p.m_hash ? (size_t)p.m_hash * 4 : 4));
  p.off_setgrp = o;  o = grouped ? o : align_up(o + (p.n ? (size_t)p.n * 4 : 4));
  p.total = o;
  return p;
}

// the new regions of the image at h (the base image's are filled by its own pack_fill)
inline void pack_fill_memo(uint8_t* h, const packed_memo& p, const group::groups& G, const resolved& R) {
  uint32_t* off = (uint32_t*)(h + p.off_hmsgoff);
  uint32_t b = 0;
  for (uint32_t j = 0; j < p.m_hash; j++) {
    const uint32_t g = R.m_hash[j];
    off[j] = b;
    if (G.len[g]) memcpy(h + p.off_hmsgs + b, G.msg[g], G.len[g]);
    b += G.len[g];
  }
  off[p.m_hash] = b;
  if (G.m) memcpy(h + p.off_src, R.src.data(), (size_t)G.m * 4);
  if (p.m_hash) memcpy(h + p.off_learn, R.learn.data(), (size_t)p.m_hash * 4);
  if (p.has_setgrp && p.n) memcpy(h + p.off_setgrp, G.set_grp.data(), (size_t)p.n * 4);
}

}  // namespace memo
}  // namespace tb
