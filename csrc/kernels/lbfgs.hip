// Master-side decode-combine + limited-memory BFGS step in ONE launch of ONE workgroup (--lbfgs M).
//
// The method (all fp64, one model of a scalar loss).  Round i holds beta_i and the decoded message sum g (the fma
// chain of combine_update, in message order); the gradient is G_i = gs g + l2c beta_i.  From round 1 on the candidate
// pair s = beta_i - beta_{i-1}, y = G_i - G_{i-1} enters a ring of `memory` pairs (the oldest is evicted) iff s.y,
// s.s and y.y are finite and s.y > 1e-8 sqrt((s.s)(y.y)); a rejected candidate leaves the ring as it was.  With k >= 1
// pairs held (oldest j = 1), rho_j = 1 / (s_j.y_j) and gamma = (s_k.y_k) / (y_k.y_k), the two-loop recursion
//     q = G_i;  j = k..1: a_j = rho_j (s_j.q), q -= a_j y_j;  q *= gamma;  j = 1..k: b = rho_j (y_j.q), q += (a_j - b) s_j
// gives p = q and beta_{i+1} = beta_i - tau p.  With no pair held the step is GD, beta_{i+1} = beta_i - eta G_i, and
// when G_i.p is not finite or not > 0 the ring is emptied and the step is GD too.
//
// Gram space.  The textbook loop is 2k DEPENDENT full-length reductions, each a pass over D and a workgroup-wide
// sum: latency the master's serial step cannot hide.  Every dot product of the recursion is an entry of Wg = V^T V
// with V = [s_1..s_k, y_1..y_k, G_i] (at most 15 columns: memory <= 7), so the kernel runs
//   phase 1  elementwise: decode g, form G_i (kept in the state's scratch row), and reduce the candidate's three
//            dot products; the acceptance is decided BEFORE the candidate is stored, because a full ring plus the
//            candidate would be 2 memory + 3 = 17 columns and an evicted pair cannot be brought back
//   phase 1b elementwise, if accepted: s and y into the ring's next slot (recomputed from the same operands)
//   phase 2  the Gram matrix on v_mfma_f64_16x16x4_f64: K = D split over the four waves in steps of 4; the lane
//            with c = lane & 15, kk = lane >> 4 loads V[k0 + kk][c] ONCE and passes that register as both the A
//            operand (V^T) and the B operand (V); unused columns and rows >= D are exact zeros; the four 16x16
//            partials are added through LDS in wave order (no atomics: bitwise reproducible)
//   phase 3  one wave: the recursion on coefficient vectors c in R^16 (q = V c, a dot with column r is (Wg c)[r]:
//            lane l holds c_l, one multiply and four cross-lane adds per dot), the descent test (Wg c)[G]
//   phase 4  elementwise: p = sum_col c[col] V[.][col] in fixed column order, beta', the worker copy, the history
//            row, beta_prev and G_prev; the scratch row keeps the step's direction (p, or G_i for a GD step)
// Head, count and the "a round has been seen" flag live in the state and are advanced here, so no host value but the
// round's coefficients enters the kernel and a captured graph of the round replays unchanged.
//
// V's column layout (fixed, so the recursion needs no index arithmetic): s_j at column j - 1, y_j at column 6 + j,
// G_i at column 14, column 15 unused.
#include <cmath>

#include "common.h"
#include "launchers.h"

namespace eh {

namespace {

using lbfgs_f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kLbfgsThreads = 256;
constexpr int kLbfgsWaves = kLbfgsThreads / 64;
constexpr int kYCol = kLbfgsMaxMemory;      // first y column
constexpr int kGCol = 2 * kLbfgsMaxMemory;  // the gradient's column

// Sum over the 64 lanes, the same bits in every lane (a butterfly of commutative adds).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over each group of 16 lanes, the same bits in every lane of the group.
__device__ __forceinline__ double sum16(double v) {
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}

}  // namespace

template <typename M, typename W>
__global__ void __launch_bounds__(kLbfgsThreads)
lbfgs_update(const CombineArgs args, const LbfgsCoefs lc, double* __restrict__ beta, double* __restrict__ hist,
             W* __restrict__ beta_w, double* __restrict__ state, int* __restrict__ ring, long long* __restrict__ stamp,
             const int* __restrict__ gate) {
  __shared__ double part[kLbfgsWaves][256];  // every wave's 16x16 partial, [reg][lane]
  __shared__ double wg[16][17];
  __shared__ double red[kLbfgsWaves][3];
  __shared__ double coef[16];
  __shared__ int mode_s;

  if (gate_closed(gate)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (stamp && tid == 0) *stamp = wall_clock64();
  const int mem = lc.memory, d = lc.d, ld = lc.ld;
  double* S = state;
  double* Y = state + static_cast<long long>(mem) * ld;
  double* bprev = state + 2LL * mem * ld;
  double* gprev = bprev + ld;
  double* gcur = gprev + ld;
  int head = ring[0], count = ring[1];
  const bool started = ring[2] != 0;
  if (head < 0 || head >= mem || count < 0 || count > mem) head = count = 0;  // a state from elsewhere: no pairs

  // ---- phase 1: decode, gradient, the candidate's dot products ------------------------------------------------
  double sy = 0.0, ss = 0.0, yy = 0.0;
  for (int c = tid; c < ld; c += kLbfgsThreads) {
    if (c >= d) {  // padded columns stay exactly zero
      if (beta_w) beta_w[c] = W(0);
      continue;
    }
    double g = 0.0;
    constexpr int kBatch = 8;  // independent loads eight at a time, accumulated in message order
    for (int m0 = 0; m0 < args.nmsg; m0 += kBatch) {
      double v[kBatch];
#pragma unroll
      for (int k = 0; k < kBatch; ++k)
        v[k] = m0 + k < args.nmsg ? static_cast<double>(static_cast<const M*>(args.msg[m0 + k])[c]) : 0.0;
#pragma unroll
      for (int k = 0; k < kBatch; ++k)
        if (m0 + k < args.nmsg) g = fma(args.coef[m0 + k], v[k], g);
    }
    const double b = beta[c];
    const double G = fma(lc.gs, g, lc.l2c * b);
    gcur[c] = G;
    if (started) {
      const double s = b - bprev[c], y = G - gprev[c];
      sy = fma(s, y, sy);
      ss = fma(s, s, ss);
      yy = fma(y, y, yy);
    }
  }
  sy = wave_sum(sy);
  ss = wave_sum(ss);
  yy = wave_sum(yy);
  if (lane == 0) {
    red[wave][0] = sy;
    red[wave][1] = ss;
    red[wave][2] = yy;
  }
  __syncthreads();
  sy = ss = yy = 0.0;
#pragma unroll
  for (int w = 0; w < kLbfgsWaves; ++w) {  // wave order: every thread forms the same three sums
    sy += red[w][0];
    ss += red[w][1];
    yy += red[w][2];
  }
  const bool accept = started && isfinite(sy) && isfinite(ss) && isfinite(yy) && sy > 1e-8 * sqrt(ss * yy);

  // ---- phase 1b: an accepted candidate enters the ring (every thread owns the columns it wrote above) ----------
  if (accept) {
    const int slot = count < mem ? (head + count) % mem : head;
    for (int c = tid; c < d; c += kLbfgsThreads) {
      S[static_cast<long long>(slot) * ld + c] = beta[c] - bprev[c];
      Y[static_cast<long long>(slot) * ld + c] = gcur[c] - gprev[c];
    }
    if (count < mem)
      ++count;
    else
      head = (head + 1) % mem;
  }
  __syncthreads();  // ring and gcur are whole

  int mode = 1;  // 0 quasi-Newton step, 1 GD step (no pair held), 2 GD step and the ring is emptied
  if (count > 0) {
    // ---- phase 2: Wg = V^T V --------------------------------------------------------------------------------
    const int vc = lane & 15, kk = lane >> 4;
    const double* col = nullptr;  // this lane's column of V
    if (vc < kYCol) {
      if (vc < count) col = S + static_cast<long long>((head + vc) % mem) * ld;
    } else if (vc < kGCol) {
      if (vc - kYCol < count) col = Y + static_cast<long long>((head + vc - kYCol) % mem) * ld;
    } else if (vc == kGCol) {
      col = gcur;
    }
    lbfgs_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int k0 = 4 * wave; k0 < d; k0 += 4 * kLbfgsWaves) {
      const int r = k0 + kk;
      const double v = (col != nullptr && r < d) ? col[r] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][r * 64 + lane] = acc[r];
    __syncthreads();
    {  // thread t owns accumulator register t / 64 of lane t % 64: row (lane >> 4) + 4 reg, column lane & 15
      double sum = 0.0;
#pragma unroll
      for (int w = 0; w < kLbfgsWaves; ++w) sum += part[w][tid];
      wg[(lane >> 4) + 4 * wave][lane & 15] = sum;
    }
    __syncthreads();

    // ---- phase 3: the two-loop recursion on coefficients, one wave ------------------------------------------
    if (wave == 0) {
      const int l = lane & 15;  // the four groups of 16 lanes compute the same thing
      double cl = l == kGCol ? 1.0 : 0.0;
      double a[kLbfgsMaxMemory], rho[kLbfgsMaxMemory];
#pragma unroll
      for (int j = kLbfgsMaxMemory - 1; j >= 0; --j) {
        a[j] = rho[j] = 0.0;
        if (j < count) {
          rho[j] = 1.0 / wg[j][kYCol + j];
          a[j] = rho[j] * sum16(wg[j][l] * cl);
          if (l == kYCol + j) cl -= a[j];
        }
      }
      const int n = kYCol + count - 1;  // the newest y
      cl *= wg[count - 1][n] / wg[n][n];
#pragma unroll
      for (int j = 0; j < kLbfgsMaxMemory; ++j)
        if (j < count) {
          const double bj = rho[j] * sum16(wg[kYCol + j][l] * cl);
          if (l == j) cl += a[j] - bj;
        }
      const double gp = sum16(wg[kGCol][l] * cl);  // G.p
      if (lane < 16) coef[lane] = cl;
      if (lane == 0) mode_s = (isfinite(gp) && gp > 0.0) ? 0 : 2;
    }
    __syncthreads();
    mode = mode_s;
  }

  // ---- phase 4: direction and step ------------------------------------------------------------------------------
  for (int c = tid; c < d; c += kLbfgsThreads) {
    const double b = beta[c], G = gcur[c];
    double nb;
    if (mode == 0) {
      double p = 0.0;
      for (int j = 0; j < count; ++j) p = fma(coef[j], S[static_cast<long long>((head + j) % mem) * ld + c], p);
      for (int j = 0; j < count; ++j) p = fma(coef[kYCol + j], Y[static_cast<long long>((head + j) % mem) * ld + c], p);
      p = fma(coef[kGCol], G, p);
      gcur[c] = p;
      nb = fma(-lc.tau, p, b);
    } else {
      nb = fma(-lc.eta, G, b);
    }
    beta[c] = nb;
    if (hist) hist[c] = nb;
    if (beta_w) beta_w[c] = static_cast<W>(nb);
    bprev[c] = b;
    gprev[c] = G;
  }
  if (tid == 0) {
    ring[0] = mode == 2 ? 0 : head;
    ring[1] = mode == 2 ? 0 : count;
    ring[2] = 1;
    ring[3] = mode;
  }
}

hipError_t lbfgs_update_launch(const CombineArgs& args, int msg_dtype, int w_dtype, double* beta, double* hist,
                               void* beta_w, double* state, int* ring, const LbfgsCoefs lc, hipStream_t st,
                               long long* stamp, const int* gate) {
  if (lc.memory < 1 || lc.memory > kLbfgsMaxMemory || lc.d < 1 || lc.d > lc.ld || !(lc.tau > 0.0) ||
      !std::isfinite(lc.tau) || args.nmsg < 0 || args.nmsg > kMaxMsgs || !beta || !state || !ring)
    return hipErrorInvalidValue;  // (a NaN tau fails the comparison)
  if ((msg_dtype != 0 && msg_dtype != 1) || (w_dtype != 0 && w_dtype != 1)) return hipErrorInvalidValue;
  auto go = [&](auto m, auto w) {
    using M = decltype(m);
    using W = decltype(w);
    hipLaunchKernelGGL((lbfgs_update<M, W>), dim3(1), dim3(kLbfgsThreads), 0, st, args, lc, beta, hist,
                       static_cast<W*>(beta_w), state, ring, stamp, gate);
    return hipGetLastError();
  };
  if (msg_dtype == 0) return w_dtype == 0 ? go(double{}, double{}) : go(double{}, float{});
  return w_dtype == 0 ? go(float{}, double{}) : go(float{}, float{});
}

}  // namespace eh
