// Host-only self test of the master's decode (decode.h), built under AddressSanitizer +
// UndefinedBehaviorSanitizer by tools/sanitize_host.sh next to the collector's.  Hand-computed cases,
// small enough to check by eye; no HIP call is ever made.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "decode.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

using eh::Arrival;
using eh::DecodeTerm;
using Terms = std::vector<DecodeTerm>;

// arrivals from (worker, part) pairs, in arrival order
static std::vector<Arrival> arrivals(const std::vector<std::pair<int, int>>& wp) {
  std::vector<Arrival> a;
  for (size_t k = 0; k < wp.size(); ++k) a.push_back({wp[k].first, wp[k].second, 0, 0.001 * k, (int)k});
  return a;
}

static bool same(const Terms& got, const Terms& want) {
  if (got.size() != want.size()) return false;
  for (size_t k = 0; k < got.size(); ++k)
    if (got[k].worker != want[k].worker || got[k].part != want[k].part || got[k].coef != want[k].coef) return false;
  return true;
}

int main() {
  const eh::DecodeTable none;
  // 1. Sum decode: every part-0 arrival with coefficient 1, in arrival order; part-1 arrivals ignored.
  {
    Terms t;
    CHECK(eh::decode_arrivals(eh::kSumPart0, {0, 1, 2, 3}, 4, none, arrivals({{2, 0}, {1, 1}, {0, 0}, {3, 1}, {3, 0}}), t));
    CHECK(same(t, {{2, 0, 1.0}, {0, 0, 1.0}, {3, 0, 1.0}}));
  }
  // 2. First per group, W = 6 in 3 groups of 2: exactly the first arrival of each group, in arrival order.
  {
    Terms t;
    CHECK(eh::decode_arrivals(eh::kFirstPerGroup, {0, 0, 1, 1, 2, 2}, 3, none,
                              arrivals({{3, 0}, {2, 0}, {5, 0}, {0, 0}, {4, 0}, {1, 0}}), t));
    CHECK(same(t, {{3, 0, 1.0}, {5, 0, 1.0}, {0, 0, 1.0}}));
  }
  // 3. Partial FRC: every part-1 message plus the first part-0 arrival of each group, interleaved as they came.
  {
    Terms t;
    CHECK(eh::decode_arrivals(eh::kPartialFrc, {0, 0, 1, 1}, 2, none,
                              arrivals({{1, 1}, {1, 0}, {0, 1}, {0, 0}, {3, 1}, {2, 1}, {2, 0}}), t));
    CHECK(same(t, {{1, 1, 1.0}, {1, 0, 1.0}, {0, 1, 1.0}, {3, 1, 1.0}, {2, 1, 1.0}, {2, 0, 1.0}}));
  }
  // 4. Table decode, W = 4, masks 0b0111 and 0b1101 present: the row's coefficients in worker order
  //    whatever the arrival order; a mask the table lacks is not decodable.
  const eh::DecodeTable table{{0b0111, {0.5, -1.0, 2.0, 9.0}}, {0b1101, {3.0, 9.0, -0.25, 1.5}}};
  {
    Terms t;
    CHECK(eh::decode_arrivals(eh::kTable, {0, 1, 2, 3}, 4, table, arrivals({{2, 0}, {0, 0}, {1, 0}}), t));
    CHECK(same(t, {{0, 0, 0.5}, {1, 0, -1.0}, {2, 0, 2.0}}));
    t.clear();
    CHECK(eh::decode_arrivals(eh::kTable, {0, 1, 2, 3}, 4, table, arrivals({{3, 0}, {2, 0}, {0, 0}}), t));
    CHECK(same(t, {{0, 0, 3.0}, {2, 0, -0.25}, {3, 0, 1.5}}));
    t.clear();
    CHECK(!eh::decode_arrivals(eh::kTable, {0, 1, 2, 3}, 4, table, arrivals({{3, 0}, {1, 0}, {0, 0}}), t));  // 0b1011
    t.clear();
    CHECK(!eh::decode_arrivals(eh::kTable, {0, 1, 2, 3}, 4, table, arrivals({{1, 1}}), t));  // mask 0: part 1 sets no bit
  }
  // 5. Partial table: the part-1 messages in arrival order, then the table's row in worker order.
  {
    Terms t;
    CHECK(eh::decode_arrivals(eh::kPartialTable, {0, 1, 2, 3}, 4, table,
                              arrivals({{3, 1}, {2, 0}, {0, 1}, {0, 0}, {1, 1}, {1, 0}, {2, 1}}), t));
    CHECK(same(t, {{3, 1, 1.0}, {0, 1, 1.0}, {1, 1, 1.0}, {2, 1, 1.0}, {0, 0, 0.5}, {1, 0, -1.0}, {2, 0, 2.0}}));
    t.clear();
    CHECK(!eh::decode_arrivals(eh::kPartialTable, {0, 1, 2, 3}, 4, table, arrivals({{3, 1}, {3, 0}, {0, 0}}), t));
  }
  // 6. Tie ranks: a permutation of 0..W-1 in every round, equal to the sort by tie_key with ties broken
  //    by worker id; all zero without a seed.
  {
    const int R = 7, W = 6;
    const int64_t seed = 1234;
    const std::vector<int> tie = eh::tie_ranks(seed, R, W);
    CHECK((int)tie.size() == R * W);
    for (int i = 0; i < R; ++i) {
      std::vector<int> seen(W, 0);
      for (int w = 0; w < W; ++w) {
        const int r = tie[i * W + w];
        CHECK(r >= 0 && r < W && !seen[r]);
        seen[r] = 1;
        int before = 0;  // workers that sort ahead of w
        for (int x = 0; x < W; ++x) {
          const uint64_t kx = eh::Collector::tie_key(seed, i, x), kw = eh::Collector::tie_key(seed, i, w);
          before += kx < kw || (kx == kw && x < w);
        }
        CHECK(r == before);
      }
    }
    for (int r : eh::tie_ranks(-1, R, W)) CHECK(r == 0);
  }
  // 7. Flattened table [2^W][W]: the rows of the two present masks hold their coefficients, every other
  //    row is NaN throughout.
  {
    const std::vector<double> flat = eh::flat_table(table, 4);
    CHECK(flat.size() == 16 * 4);
    for (uint64_t mask = 0; mask < 16; ++mask)
      for (int w = 0; w < 4; ++w) {
        const double v = flat[mask * 4 + w];
        auto it = table.find(mask);
        if (it == table.end())
          CHECK(std::isnan(v));
        else
          CHECK(v == it->second[w]);
      }
    CHECK(std::count_if(flat.begin(), flat.end(), [](double v) { return std::isnan(v); }) == 14 * 4);
  }
  std::printf("decode selftest ok\n");
  return 0;
}
