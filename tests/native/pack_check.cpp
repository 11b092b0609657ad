// CPU check of the staging image of a host batch (teku_amd/csrc/tb_pack.h;
// tests/test_pack.py).  For each case: pack_layout, then pack_fill into a heap
// block of exactly `total` bytes pre-filled with the marker byte 0xA5 (so ASan
// sees a write past the image), then one line
//   case <name> n=<n> K=<K> M=<M> off=<the seven region offsets> total=<total> image=<hex>
// The inputs are the byte patterns below; tests/test_pack.py generates the
// same inputs and builds the expected image from the format's statement.
#include <cstdio>
#include <string>
#include <vector>

#include "tb_pack.h"

using namespace tb::pack;

static const uint8_t MARK = 0xA5;

// input bytes: field `tag` (1 keys, 2 message, 3 signature, 4 DST) of set i, byte j
static uint8_t pat(uint32_t tag, uint32_t i, uint32_t j) { return (uint8_t)(tag * 61u + i * 17u + j * 7u + 3u); }

struct input {
  std::vector<std::vector<uint8_t>> keys, msgs, sigs;  // per set
  std::vector<uint64_t> rand;
  std::vector<uint8_t> dst;
};

// n sets; set i has n_keys[i] key bytes (already in the set kind's unit) and msg_len[i] message bytes
static input make_input(const std::vector<uint32_t>& key_len, const std::vector<uint32_t>& msg_len, uint32_t dlen) {
  input in;
  for (uint32_t i = 0; i < key_len.size(); i++) {
    std::vector<uint8_t> k(key_len[i]), m(msg_len[i]), s(96);
    for (uint32_t j = 0; j < k.size(); j++) k[j] = pat(1, i, j);
    for (uint32_t j = 0; j < m.size(); j++) m[j] = pat(2, i, j);
    for (uint32_t j = 0; j < 96; j++) s[j] = pat(3, i, j);
    in.keys.push_back(k);
    in.msgs.push_back(m);
    in.sigs.push_back(s);
    in.rand.push_back(0x0102030405060708ull * (i + 1) + i);
  }
  in.dst.resize(dlen);
  for (uint32_t j = 0; j < dlen; j++) in.dst[j] = pat(4, 0, j);
  return in;
}

template <class SET>
static void emit(const char* name, const std::vector<SET>& sets, size_t lo, size_t hi, const uint64_t* rand, const input& in) {
  const uint32_t dlen = (uint32_t)in.dst.size();
  const packed p = pack_layout(sets.data(), lo, hi, dlen);
  uint8_t* h = new uint8_t[p.total];
  memset(h, MARK, p.total);
  pack_fill(h, p, sets.data(), lo, rand, dlen ? in.dst.data() : nullptr, dlen);
  printf("case %s n=%u K=%u M=%u off=%zu,%zu,%zu,%zu,%zu,%zu,%zu total=%zu image=", name, p.n, p.K, p.M, p.off_pks, p.off_pkoff, p.off_msgs,
         p.off_msgoff, p.off_sigs, p.off_rand, p.off_dst, p.total);
  for (size_t i = 0; i < p.total; i++) printf("%02x", h[i]);
  printf("\n");
  delete[] h;
}

static const uint8_t* ptr(const std::vector<uint8_t>& v) { return v.empty() ? nullptr : v.data(); }

int main() {
  {  // an empty range
    const input in = make_input({}, {}, 43);
    emit("empty", std::vector<tbls_set>(), 0, 0, nullptr, in);
  }
  {  // one set with one key, an empty message and no DST, no randomizers
    const input in = make_input({48}, {0}, 0);
    std::vector<tbls_set> s = {{ptr(in.keys[0]), 1, nullptr, 0, in.sigs[0].data()}};
    emit("one", s, 0, 1, nullptr, in);
  }
  {  // [1, 3) of three sets with 1 / 2 / 3 keys and messages of 0 / 1 / 300 bytes, randomizers given: as byte keys, as indices
    const std::vector<uint32_t> nk = {1, 2, 3}, ml = {0, 1, 300};
    const input a = make_input({48, 96, 144}, ml, 43), b = make_input({4, 8, 12}, ml, 43);
    std::vector<tbls_set> sa;
    std::vector<tbls_set_idx> sb;
    for (int i = 0; i < 3; i++) {
      sa.push_back({a.keys[i].data(), nk[i], ptr(a.msgs[i]), ml[i], a.sigs[i].data()});
      sb.push_back({(const uint32_t*)b.keys[i].data(), nk[i], ptr(b.msgs[i]), ml[i], b.sigs[i].data()});
    }
    emit("bytes_1_3", sa, 1, 3, a.rand.data(), a);
    emit("idx_1_3", sb, 1, 3, b.rand.data(), b);
  }
  for (uint32_t size : {13u, 512u}) {  // bit rows over a committee of `size` members: two sets, no randomizers
    const uint32_t nb = (size + 7) / 8;
    const input in = make_input({nb, nb}, {32, 5}, 43);
    std::vector<set_bits_i> s;
    for (int i = 0; i < 2; i++) s.push_back({in.keys[i].data(), bits_stride_w(size), in.msgs[i].data(), (uint32_t)in.msgs[i].size(), in.sigs[i].data(), 0, size});
    emit(size == 13 ? "bits_13" : "bits_512", s, 0, 2, nullptr, in);
  }
  return 0;
}
