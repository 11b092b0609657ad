// CPU check of the hash-point memo's host index (teku_amd/csrc/tb_msgmemo.h;
// tests/test_msgmemo_host.py).  Reads a script (argv[1]) of lines
//   rows <R>                  configure the index
//   shard <msg> <msg> ...     one set per message, hex bytes ("-": the empty message); per_set pairs
//   gshard <msg> <msg> ...    the same through a grouped pass (one pair per distinct message)
//   invalidate
// and prints after every shard one line
//   m_hash=<groups> src=<words> learn=<words> flushed=<0|1> hits=<n> hashed=<n> flushes=<n> used=<n>
// (a list of no entries prints as "-"; words in hex).  Every message is a heap
// copy of exactly its length, so ASan sees a read past a message, and the
// copies are freed before the next line: the index must keep its own bytes.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tb_msgmemo.h"

static void list(const char* name, const std::vector<uint32_t>& v) {
  printf("%s=", name);
  if (v.empty()) printf("-");
  for (size_t i = 0; i < v.size(); i++) printf("%s%x", i ? "," : "", v[i]);
  printf(" ");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  tb::memo::index X;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string op;
    ls >> op;
    if (op == "rows") {
      uint32_t r;
      ls >> r;
      X.configure(r);
    } else if (op == "invalidate") {
      X.invalidate();
    } else if (op == "shard" || op == "gshard") {
      std::vector<uint8_t*> heap;
      std::vector<tbls_set> sets;
      std::string tok;
      while (ls >> tok) {
        const size_t len = tok == "-" ? 0 : tok.size() / 2;
        uint8_t* p = new uint8_t[len ? len : 1];
        for (size_t i = 0; i < len; i++) p[i] = (uint8_t)std::stoi(tok.substr(2 * i, 2), nullptr, 16);
        heap.push_back(p);
        sets.push_back({nullptr, 1, len ? p : nullptr, (uint32_t)len, nullptr});
      }
      const tb::memo::resolved R = X.resolve(sets.data(), 0, sets.size(), op == "shard");
      for (uint8_t* p : heap) delete[] p;
      list("m_hash", R.m_hash);
      list("src", R.src);
      list("learn", R.learn);
      printf("flushed=%d hits=%llu hashed=%llu flushes=%llu used=%u\n", (int)R.flushed, (unsigned long long)X.hits, (unsigned long long)X.hashed,
             (unsigned long long)X.flushes, X.used);
    } else if (!op.empty()) {
      return 3;
    }
  }
  return 0;
}
