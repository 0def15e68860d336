// Host decode of a round's arrivals and the two tables the device arbiter copies (arbiter.h): pure
// logic on the collector's arrivals -- no HIP call, no torch, no pybind -- so a host self test
// (decode_selftest.cpp) checks it without a GPU.  MasterPump maps the decoded terms to buffer rows.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "collector.h"

namespace eh {

// Decode kinds (codes/schemes.py DEC_*; tests/test_native_enums.py pins the two copies together)
enum DecodeKind : int {
  kSumPart0 = 0,       // naive, avoidstragg: every arrived main message, coefficient 1
  kFirstPerGroup = 1,  // FRC / AGC: first arrival of each group
  kPartialFrc = 2,     // partial replication: all first parts + first second part per group
  kTable = 3,          // cyclic MDS: coefficients from the completion-bitmask table
  kPartialTable = 4,   // partial coded: all first parts + table-decoded coded parts
};
inline bool table_decode(int kind) { return kind == kTable || kind == kPartialTable; }

using DecodeTable = std::map<uint64_t, std::vector<double>>;  // completion bitmask -> [W] coefficients

// One message a decode uses.
struct DecodeTerm {
  int worker, part;
  double coef;
};

// The messages round `arr` decodes to, in the order the combine adds them: part-1 messages and sum / group
// picks interleaved in arrival order, then the table's coefficients in worker order.  False: the
// completion pattern is not in the table (`out` is then meaningless).
inline bool decode_arrivals(int kind, const std::vector<int>& group_of, int n_groups, const DecodeTable& table,
                            const std::vector<Arrival>& arr, std::vector<DecodeTerm>& out) {
  std::vector<char> gdone(std::max(n_groups, 1), 0);
  uint64_t mask = 0;
  for (const auto& a : arr) {
    if (a.part == 1) {
      if (kind == kPartialFrc || kind == kPartialTable) out.push_back({a.worker, 1, 1.0});
      continue;
    }
    switch (kind) {
      case kSumPart0:
        out.push_back({a.worker, 0, 1.0});
        break;
      case kFirstPerGroup:
      case kPartialFrc: {
        const int g = group_of[a.worker];
        if (!gdone[g]) {
          gdone[g] = 1;
          out.push_back({a.worker, 0, 1.0});
        }
        break;
      }
      default:
        mask |= (uint64_t)1 << a.worker;
    }
  }
  if (table_decode(kind)) {
    auto it = table.find(mask);
    if (it == table.end()) return false;
    for (int w = 0; w < (int)group_of.size(); ++w)
      if (mask >> w & 1) out.push_back({w, 0, it->second[w]});
  }
  return true;
}

// [R][W] rank of every worker in each round's tie permutation (Collector::tie_key, ties by worker id);
// all zero for seed < 0 (ties keep probe order).
inline std::vector<int> tie_ranks(int64_t seed, int R, int W) {
  std::vector<int> tie(static_cast<size_t>(R) * W, 0);
  if (seed < 0) return tie;
  std::vector<int> ord(W);
  for (int i = 0; i < R; ++i) {
    for (int w = 0; w < W; ++w) ord[w] = w;
    std::sort(ord.begin(), ord.end(), [&](int x, int y) {
      const uint64_t kx = Collector::tie_key(seed, i, x), ky = Collector::tie_key(seed, i, y);
      return kx != ky ? kx < ky : x < y;
    });
    for (int r = 0; r < W; ++r) tie[static_cast<size_t>(i) * W + ord[r]] = r;
  }
  return tie;
}

// The table as dense rows [2^W][W]; NaN in the rows of masks it does not hold.
inline std::vector<double> flat_table(const DecodeTable& table, int W) {
  std::vector<double> flat((size_t{1} << W) * W, std::nan(""));
  for (const auto& [mask, coefs] : table)
    if (mask < (uint64_t{1} << W))
      for (int w = 0; w < W; ++w) flat[mask * W + w] = coefs[w];
  return flat;
}

}  // namespace eh
