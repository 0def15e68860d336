// Exact ROC AUC pair counts of every column of a prediction matrix: LDS tile sort + binary-search count (K11).
//
// For a column with scores s, the rows of one class ("sorted", m of them) and the rows of the other ("queries", nq):
//   sum = sum over queries q of ( #{sorted keys < q} + #{sorted keys <= q} )
// an exact integer.  With the negatives sorted it is U2 = sum_{p in Pos} (2 #{neg < p} + #{neg == p}); with the
// positives sorted U2 = 2 m nq - sum; AUC = U2 / (2 n+ n-), ties counting 1/2 by construction (ops/eval.py divides).
// Only the order between the two classes matters, so nothing is ranked and nothing is sorted globally: the counts of
// the sorted class's tiles add up.
//
// 1. auc_keys (once per class): gathers the rows of one class from P [n, ldp] (fp64 or fp32) through the class's row
//    list and writes their keys column-major, K[column][slot].  A 64 x 64 tile goes through LDS, so a wave reads 64
//    neighbouring columns of one row and writes 64 neighbouring slots of one column.  The key is the order-preserving
//    unsigned image of the score widened to fp64 (sign bit flipped for positives, all bits for negatives), -0.0 taken
//    as +0.0 first; the test for zero and NaN is on the bits, so no floating-point mode enters.  A NaN raises the
//    column's flag word (every writer stores the same 1).  Slots [m, tiles * T) of the sorted class are written as the
//    all-ones key, so a count workgroup loads whole tiles.
// 2. auc_count: one workgroup of 1024 threads per (tile t of T sorted keys, column j).  The tile is sorted in LDS by a
//    bitonic network over the next power of two >= its real key count (padding sorts to the end), then all queries of
//    the column stream through with coalesced loads, four per thread at a time so that their LDS probes overlap: a
//    branch-free binary search over the REAL keys of the tile gives lb = #keys < q (the same number of probes in every
//    lane); only where keys[lb] == q does a second search over [lb, count) find ub = #keys <= q, otherwise ub = lb.
//    Every thread adds lb + ub into a 64-bit integer; lanes are added by shuffles, the 16 waves through LDS in wave
//    order, one store to part[j][t].  No atomics, no floating point: the result does not depend on the launch
//    geometry.
// 3. auc_sum: sums[j] = part[j][0] + part[j][1] + ... in tile order.
//
// Work per column: nq * ceil(m / T) searches of log2 T probes, all in LDS; the queries are re-read once per tile.
#include <cstdint>

#include "launchers.h"

namespace eh {
namespace {

using u64 = unsigned long long;

constexpr int kKeyTile = 64;  // slots x columns of one transpose tile: 4 waves, a wave per row / column of it
constexpr int kCountThreads = 1024;
constexpr int kCountWaves = kCountThreads / 64;
constexpr int kCountQueries = 4;  // queries a thread searches at once

template <class F>
__device__ __forceinline__ u64 score_key(F v, bool& nan) {
  u64 b = static_cast<u64>(__double_as_longlong(static_cast<double>(v)));
  const u64 mag = b & 0x7fffffffffffffffull;
  nan = mag > 0x7ff0000000000000ull;
  if (mag == 0) b = 0;  // -0.0 == +0.0
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void auc_clear(int* flags, int ncols) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < ncols) flags[j] = 0;
}

// K[c][slot] = key(P[rows[slot]][c]) for slot < nreal, all-ones for nreal <= slot < nout; c < ncols.
template <class F, class I>
__global__ __launch_bounds__(256) void auc_keys(const F* __restrict__ P, long long ldp, const I* __restrict__ rows,
                                                long long nreal, long long nout, int ncols, u64* __restrict__ K,
                                                long long ldk, int* flags) {
  __shared__ u64 tile[kKeyTile][kKeyTile + 1];
  const long long s0 = static_cast<long long>(blockIdx.x) * kKeyTile;
  const int c0 = blockIdx.y * kKeyTile;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = c0 + tx;  // reading: the lane is the column
  bool any_nan = false;
  for (int s = ty; s < kKeyTile; s += 4) {
    const long long slot = s0 + s;
    u64 key = ~0ull;
    if (slot < nreal && c < ncols) {
      bool nan;
      key = score_key(P[static_cast<long long>(rows[slot]) * ldp + c], nan);
      any_nan |= nan;
    }
    tile[s][tx] = key;
  }
  if (any_nan) flags[c] = 1;
  __syncthreads();
  const long long slot = s0 + tx;  // writing: the lane is the slot
  if (slot < nout)
    for (int cc = ty; cc < kKeyTile && c0 + cc < ncols; cc += 4)
      K[static_cast<long long>(c0 + cc) * ldk + slot] = tile[tx][cc];
}

// base + #keys[base .. base + count) that are <= x; count >= 1, keys ascending.  The trip count depends on count
// alone; auc_count runs the same search with < for the lower bounds of kCountQueries queries at once.
__device__ __forceinline__ int count_le(const u64* keys, int base, int count, u64 x) {
  while (count > 1) {
    const int half = count >> 1;
    if (keys[base + half - 1] <= x) base += half;
    count -= half;
  }
  return base + (keys[base] <= x ? 1 : 0);
}

// S [ncols][lds_] with lds_ = tiles * T (padded), Q [ncols][nq], part [ncols][tiles]; grid (tiles, ncols)
__global__ __launch_bounds__(kCountThreads) void auc_count(const u64* __restrict__ S, long long lds_, long long m,
                                                           const u64* __restrict__ Q, long long nq, int T,
                                                           u64* __restrict__ part) {
  extern __shared__ u64 keys[];  // [T]
  __shared__ u64 wsum[kCountWaves];
  const int tid = threadIdx.x;
  const int t = blockIdx.x, j = blockIdx.y;
  const long long first = static_cast<long long>(t) * T;
  const int count = static_cast<int>(m - first < T ? m - first : T);  // real keys of this tile, >= 1
  int N = 2;
  while (N < count) N <<= 1;  // <= T: T is a power of two
  const u64* s = S + static_cast<long long>(j) * lds_ + first;
  for (int i = tid; i < N; i += kCountThreads) keys[i] = s[i];
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1) {
    for (int d = k >> 1; d > 0; d >>= 1) {
      for (int i = tid; i < (N >> 1); i += kCountThreads) {
        const int a = ((i & ~(d - 1)) << 1) | (i & (d - 1)), b = a | d;
        const u64 x = keys[a], y = keys[b];
        if ((x > y) == ((a & k) == 0)) {
          keys[a] = y;
          keys[b] = x;
        }
      }
      __syncthreads();
    }
  }
  u64 acc = 0;
  const u64* q = Q + static_cast<long long>(j) * nq;
  // kCountQueries searches in flight per thread: their probes are independent, so LDS latency overlaps
  for (long long i0 = tid; i0 < nq; i0 += kCountThreads * kCountQueries) {
    u64 x[kCountQueries];
    int base[kCountQueries];
#pragma unroll
    for (int u = 0; u < kCountQueries; ++u) {
      const long long i = i0 + static_cast<long long>(u) * kCountThreads;
      x[u] = i < nq ? q[i] : 0;
      base[u] = 0;
    }
    int left = count;
    while (left > 1) {  // count_le's loop with <, for all of them step by step
      const int half = left >> 1;
#pragma unroll
      for (int u = 0; u < kCountQueries; ++u)
        if (keys[base[u] + half - 1] < x[u]) base[u] += half;
      left -= half;
    }
#pragma unroll
    for (int u = 0; u < kCountQueries; ++u) {
      const int lb = base[u] + (keys[base[u]] < x[u] ? 1 : 0);
      int ub = lb;
      if (lb < count && keys[lb] == x[u]) ub = count_le(keys, lb, count - lb, x[u]);
      if (i0 + static_cast<long long>(u) * kCountThreads < nq) acc += static_cast<u64>(lb + ub);
    }
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((tid & 63) == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    u64 total = 0;
    for (int w = 0; w < kCountWaves; ++w) total += wsum[w];
    part[static_cast<long long>(j) * gridDim.x + t] = total;
  }
}

__global__ __launch_bounds__(256) void auc_sum(const u64* __restrict__ part, int tiles, int ncols, long long* sums) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ncols) return;
  u64 total = 0;
  for (int t = 0; t < tiles; ++t) total += part[static_cast<long long>(j) * tiles + t];
  sums[j] = static_cast<long long>(total);
}

template <class F, class I>
hipError_t launch_keys(const void* P, long long ldp, const void* rows, long long nreal, long long nout, int ncols,
                       u64* K, long long ldk, int* flags, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>((nout + kKeyTile - 1) / kKeyTile),
                  static_cast<unsigned>((ncols + kKeyTile - 1) / kKeyTile));
  hipLaunchKernelGGL((auc_keys<F, I>), grid, dim3(256), 0, st, static_cast<const F*>(P), ldp,
                     static_cast<const I*>(rows), nreal, nout, ncols, K, ldk, flags);
  return hipGetLastError();
}

}  // namespace

hipError_t auc_pair_sums_launch(int p_dtype, int idx64, const void* P, long long ldp, const void* rows_sorted,
                                long long m, const void* rows_query, long long nq, int ncols, int T,
                                unsigned long long* S, unsigned long long* Q, unsigned long long* part,
                                long long* sums, int* flags, hipStream_t st) {
  if (p_dtype != 0 && p_dtype != 1) return hipErrorInvalidValue;
  if (T < 2 || T > kAucMaxTile || (T & (T - 1)) != 0) return hipErrorInvalidValue;
  if (m < 1 || nq < 1 || m + nq > 0x7fffffffLL || ncols < 0 || ldp < ncols) return hipErrorInvalidValue;
  if (ncols == 0) return hipSuccess;
  const long long tiles = auc_tiles(m, T);
  // grid.y is the column; the whole grid stays below 2^31 threads
  if (ncols > 65535 || tiles * ncols * kCountThreads > 0x7fffffffLL) return hipErrorInvalidValue;
  const long long key_blocks = ((tiles * T > nq ? tiles * T : nq) / kKeyTile + 1) * (ncols / kKeyTile + 1);
  if (key_blocks * 256 > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(auc_clear, dim3((ncols + 255) / 256), dim3(256), 0, st, flags, ncols);
  auto keys = [&](const void* rows, long long nreal, long long nout, u64* K) {
    if (p_dtype == 0)
      return idx64 ? launch_keys<double, long long>(P, ldp, rows, nreal, nout, ncols, K, nout, flags, st)
                   : launch_keys<double, int>(P, ldp, rows, nreal, nout, ncols, K, nout, flags, st);
    return idx64 ? launch_keys<float, long long>(P, ldp, rows, nreal, nout, ncols, K, nout, flags, st)
                 : launch_keys<float, int>(P, ldp, rows, nreal, nout, ncols, K, nout, flags, st);
  };
  if (const hipError_t e = keys(rows_sorted, m, tiles * T, S); e != hipSuccess) return e;
  if (const hipError_t e = keys(rows_query, nq, nq, Q); e != hipSuccess) return e;
  const size_t lds = static_cast<size_t>(T) * sizeof(u64);
  if (const hipError_t e = allow_dynamic_lds(auc_count, lds, sizeof(u64) * kCountWaves); e != hipSuccess) return e;
  hipLaunchKernelGGL(auc_count, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(ncols)), dim3(kCountThreads),
                     lds, st, S, tiles * T, m, Q, nq, T, part);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(auc_sum, dim3((ncols + 255) / 256), dim3(256), 0, st, part, static_cast<int>(tiles), ncols, sums);
  return hipGetLastError();
}

}  // namespace eh
