// The descent of settling a failed batch (tb_lib.hip settle_tail): which
// groups of the n per-set Miller values are tested, in what order, and what
// the tests make of each set -- as plain host code over a tester callback.  No
// HIP: tests/native/settle_descent_check.cpp compiles this header with g++ and
// drives it with a simulated tester.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "tb_plan.h"

namespace tb {
namespace plan {

// What a tested index names: a level-B group (TB_SETTLE_FAN level-A groups),
// a level-A group (TB_SETTLE_FAN values), or one value.
enum settle_level { SETTLE_LEAF = 0, SETTLE_A = 1, SETTLE_B = 2 };

// ok[0..S.n) from group tests, top level first: every level-B group, then the
// level-A groups of the B groups that fail, then of the A groups that fail the
// values whose code is 0 (codes[i] != 0: value i's set is invalid by its code
// alone; its value is 1, so it fails no group).  A set is valid when its code
// is 0 and its B group, its A group or its own value passes.
// test(level, list, pass): 0, or an error code that ends the descent;
// pass[k] = 1 iff index list[k] of `level` tests 1.  list is ascending and
// never empty, pass comes sized to it and zeroed.
template <class TEST>
int settle_descent(const settle_layout& S, const std::vector<uint8_t>& codes, uint8_t* ok, const TEST& test) {
  const uint32_t F = TB_SETTLE_FAN, n = S.n;
  std::vector<uint8_t> passB(S.nB, 0), passA(S.nA, 0), leaf(n, 0), pass;
  std::vector<uint32_t> list, open;  // the level under test; the members of its failing groups
  // test `list` at `level`, the verdicts into dst by index
  const auto run = [&](settle_level level, std::vector<uint8_t>& dst) {
    if (list.empty()) return 0;
    pass.assign(list.size(), 0);
    if (const int rc = test(level, list, pass)) return rc;
    for (size_t k = 0; k < list.size(); k++) dst[list[k]] = pass[k];
    return 0;
  };
  for (uint32_t b = 0; b < S.nB; b++) list.push_back(b);
  if (const int rc = run(SETTLE_B, passB)) return rc;
  for (uint32_t b : list)
    if (!passB[b])
      for (uint32_t a = b * F; a < std::min(S.nA, (b + 1) * F); a++) open.push_back(a);
  list.swap(open);
  if (const int rc = run(SETTLE_A, passA)) return rc;
  open.clear();
  for (uint32_t a : list)
    if (!passA[a])
      for (uint32_t i = a * F; i < std::min(n, (a + 1) * F); i++)
        if (codes[i] == 0) open.push_back(i);
  list.swap(open);
  if (const int rc = run(SETTLE_LEAF, leaf)) return rc;
  for (uint32_t i = 0; i < n; i++) ok[i] = codes[i] == 0 && (passB[i / F / F] || passA[i / F] || leaf[i]) ? 1 : 0;
  return 0;
}

}  // namespace plan
}  // namespace tb
