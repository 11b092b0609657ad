// The staging image of a host batch: sets[lo, hi) of a tbls_set / tbls_set_idx
// / bit-row array packed into one contiguous block that is copied to the
// device in one piece and read there by the kernels through its offsets -- an
// offset / stride contract with them.  Plain host code, no HIP:
// tests/native/pack_check.cpp compiles this header with g++ and
// tests/test_pack.py compares the images byte for byte with the format below.
// Not included by any kernel translation unit.
//
// Regions, in this order, each starting at a multiple of 256 bytes:
//   keys         the sets' keys back to back: 48-byte encodings, 4-byte table
//                indices, or per set one participation bit row, zero-padded
//                to the call's row stride in 4-byte words
//   key offsets  n + 1 words: set i's keys are [off[i], off[i + 1]), counted
//                in keys (bit rows: in words) from the start of this image
//   messages     the sets' messages back to back (1 byte when all are empty)
//   msg offsets  n + 1 words, in bytes
//   signatures   n x 96 bytes
//   randomizers  n x 8 bytes: rand[lo + i], or 1 when the call gives none
//   DST          dlen bytes (1 byte when dlen is 0)
// Bytes between a region's end and the next region are not written.
#pragma once
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "../../include/tekubls.h"
#include "tb_plan.h"  // align_up

namespace tb {
namespace pack {

using plan::align_up;

// A bitfield set inside the library: n_pks is its row in the key area, in
// 4-byte words (the stride of every row of the call); size: the committee's
// size the caller saw (checked again under the device lock).
struct set_bits_i {
  const uint8_t* bits;
  uint32_t n_pks;
  const uint8_t* msg;
  uint32_t msg_len;
  const uint8_t* sig;
  uint32_t slot, size;
};
inline uint32_t bits_stride_w(uint32_t size) { return (size + 31u) / 32u; }  // the (size + 7) / 8 bytes, rounded to 4

// keys of a set: 48-byte encodings (tbls_set), else 4-byte table indices
// (tbls_set_idx) or words of a bit row (set_bits_i)
template <class SET>
constexpr size_t key_bytes() { return std::is_same<SET, tbls_set>::value ? 48 : 4; }

inline void pack_keys(uint8_t* dst, const tbls_set& s) {
  if (s.n_pks) memcpy(dst, s.pks, (size_t)s.n_pks * 48);
}
inline void pack_keys(uint8_t* dst, const tbls_set_idx& s) {
  if (s.n_pks) memcpy(dst, s.key_idx, (size_t)s.n_pks * 4);
}
inline void pack_keys(uint8_t* dst, const set_bits_i& s) {  // the bit row, zero-padded to its stride
  memset(dst, 0, (size_t)s.n_pks * 4);
  memcpy(dst, s.bits, (s.size + 7u) / 8u);
}

struct packed {
  size_t off_pks, off_pkoff, off_msgs, off_msgoff, off_sigs, off_rand, off_dst, total;
  uint32_t n, K, M;  // sets, keys (bit rows: words), message bytes
};

template <class SET>
packed pack_layout(const SET* sets, size_t lo, size_t hi, uint32_t dlen) {
  packed p;
  p.n = (uint32_t)(hi - lo);
  uint64_t K = 0, M = 0;
  for (size_t i = lo; i < hi; i++) {
    K += sets[i].n_pks;
    M += sets[i].msg_len;
  }
  p.K = (uint32_t)K;
  p.M = (uint32_t)M;
  size_t o = 0;
  p.off_pks = o;    o = align_up(o + (size_t)K * key_bytes<SET>());
  p.off_pkoff = o;  o = align_up(o + ((size_t)p.n + 1) * 4);
  p.off_msgs = o;   o = align_up(o + (M ? M : 1));
  p.off_msgoff = o; o = align_up(o + ((size_t)p.n + 1) * 4);
  p.off_sigs = o;   o = align_up(o + (size_t)p.n * 96);
  p.off_rand = o;   o = align_up(o + (size_t)p.n * 8);
  p.off_dst = o;    o = align_up(o + (dlen ? dlen : 1));
  p.total = o;
  return p;
}

// the image of sets[lo, lo + p.n) at h (p.total bytes); rand (nullable) is indexed like sets
template <class SET>
void pack_fill(uint8_t* h, const packed& p, const SET* sets, size_t lo, const uint64_t* rand, const uint8_t* dst, uint32_t dlen) {
  uint32_t* pkoff = (uint32_t*)(h + p.off_pkoff);
  uint32_t* moff = (uint32_t*)(h + p.off_msgoff);
  uint64_t* rr = (uint64_t*)(h + p.off_rand);
  uint32_t k = 0, m = 0;
  for (uint32_t i = 0; i < p.n; i++) {
    const SET& s = sets[lo + i];
    pkoff[i] = k;
    moff[i] = m;
    pack_keys(h + p.off_pks + (size_t)k * key_bytes<SET>(), s);
    if (s.msg_len) memcpy(h + p.off_msgs + m, s.msg, s.msg_len);
    memcpy(h + p.off_sigs + (size_t)i * 96, s.sig, 96);
    rr[i] = rand ? rand[lo + i] : 1;
    k += s.n_pks;
    m += s.msg_len;
  }
  pkoff[p.n] = k;
  moff[p.n] = m;
  if (dlen) memcpy(h + p.off_dst, dst, dlen);
}

}  // namespace pack
}  // namespace tb
