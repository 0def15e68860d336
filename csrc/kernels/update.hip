// Master-side decode-combine + GD/AGD model update in ONE launch (K5 + K7 + K8 of SURVEY §2.8).
//
// Reference semantics:
//   combine   g = sum_m a_m * msg_m                      ref src/coded.py:147-149 (lstsq decode),
//                                                        src/approximate_coding.py:150-158 (FRC first-per-group),
//                                                        src/naive.py:109 (plain sum)
//   GD        beta = (1 - 2 alpha eta) beta - (eta/n) g   ref src/naive.py:112-115
//   AGD       theta = 2/(i+2); y = (1-theta) beta + theta u
//             beta' = y - (eta/n) g - 2 alpha eta beta; u = beta + (beta'-beta)/theta   ref src/naive.py:116-122
//             (avoidstragg rescales eta/n by W/(W-s): ref src/avoidstragg.py:116)
//
// The decode coefficients a_m (fp64, solved on the host) and the message pointers are
// passed by value in the kernel arguments, so a round's combine+update is a single
// launch with no host->device copies.  Every column is independent: a thread per
// column streams the m message rows (coalesced), keeps everything in fp64 registers
// and writes beta, u, the betaset history row and the worker-dtype copy of beta that
// the next round's gradient kernels (and the p2p sends) read.
#include "common.h"
#include "launchers.h"

namespace eh {

template <typename M, typename W>
__global__ void __launch_bounds__(256)
combine_update(const CombineArgs args, double* __restrict__ beta, double* __restrict__ u,
               double* __restrict__ hist, W* __restrict__ beta_w, double* __restrict__ g_out,
               int d, int ld, double decay, double gm, double l2, double theta, int rule,
               long long* __restrict__ stamp) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (stamp && c == 0) *stamp = wall_clock64();  // device time the round's messages were all ready
  if (c >= ld) return;
  if (c >= d) {  // padded columns stay exactly zero
    if (beta_w) beta_w[c] = W(0);
    return;
  }
  // The message rows are independent loads (remote ones in fine-grained memory, ~µs each): issue
  // them eight at a time, then accumulate in message order (the same fma chain, bitwise, as a
  // one-at-a-time loop).
  double g = 0.0;
  constexpr int kBatch = 8;
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
  double nb;
  if (rule == 0) {  // GD
    nb = decay * b - gm * g;
  } else {  // AGD (gradient evaluated at beta, exactly as the reference)
    const double yt = (1.0 - theta) * b + theta * u[c];
    nb = yt - gm * g - l2 * b;
    u[c] = b + (nb - b) * (1.0 / theta);
  }
  beta[c] = nb;
  if (hist) hist[c] = nb;
  if (beta_w) beta_w[c] = static_cast<W>(nb);
  if (g_out) g_out[c] = g;
}

// Soft threshold, the proximal operator of t * |x|.  NaN fails the comparison and stays NaN, +-inf stays
// +-inf, and every |x| <= t (-0.0 at t = 0 included) becomes +0.0.
__device__ __forceinline__ double soft_threshold(double x, double t) {
  return fabs(x) <= t ? 0.0 : x - copysign(t, x);
}

// combine_update for a model of several blocks with per-block coefficients C (launchers.h BlockCoefs or ProxCoefs):
// the same batched message loads, the same fma chain and the same update expressions, so with BlockCoefs block k is
// bitwise what combine_update gives on that block alone with (decay_k, gm_k, l2_k).  With ProxCoefs the proximal
// step of an L1 penalty follows, beta' = S_thr(beta'), and the AGD momentum u is formed from the thresholded beta';
// a single model is one block.  One kernel text, written out here and not in helpers shared with combine_update:
// the BlockCoefs and ProxCoefs instantiations have to stay the code of the two kernels this one replaced
// (docs/PERF_NOTES.md "Blocked-model consolidation").
template <typename M, typename W, typename C>
__global__ void __launch_bounds__(256)
combine_update_blocked(const CombineArgs args, const C bc, double* __restrict__ beta, double* __restrict__ u,
                       double* __restrict__ hist, W* __restrict__ beta_w, double* __restrict__ g_out, double theta,
                       int rule, long long* __restrict__ stamp) {
  constexpr bool kProx = std::is_same_v<C, ProxCoefs>;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (stamp && c == 0) *stamp = wall_clock64();
  if (c >= bc.nblocks * bc.block_ld) return;
  const int blk = c / bc.block_ld;
  if (c - blk * bc.block_ld >= bc.d_x) {  // padded columns of every block stay exactly zero
    if (beta_w) beta_w[c] = W(0);
    return;
  }
  double decay = bc.decay[0], gm = bc.gm[0], l2 = bc.l2[0], thr = 0.0;
  if constexpr (kProx) thr = bc.thr[0];
#pragma unroll
  for (int k = 1; k < kMaxBlocks; ++k)  // selects, not a dynamically indexed copy of the argument
    if (k == blk) {
      decay = bc.decay[k];
      gm = bc.gm[k];
      l2 = bc.l2[k];
      if constexpr (kProx) thr = bc.thr[k];
    }
  double g = 0.0;
  constexpr int kBatch = 8;
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
  double nb;
  if (rule == 0) {  // GD
    nb = decay * b - gm * g;
    if constexpr (kProx) nb = soft_threshold(nb, thr);
  } else {  // AGD
    const double yt = (1.0 - theta) * b + theta * u[c];
    nb = yt - gm * g - l2 * b;
    if constexpr (kProx) nb = soft_threshold(nb, thr);
    u[c] = b + (nb - b) * (1.0 / theta);
  }
  beta[c] = nb;
  if (hist) hist[c] = nb;
  if (beta_w) beta_w[c] = static_cast<W>(nb);
  if (g_out) g_out[c] = g;
}

namespace {

// f(M, W) for the message and worker-beta types of two dtype codes (0 fp64, 1 fp32); any other code launches nothing.
template <class F>
hipError_t dispatch_msg_w(int msg_dtype, int w_dtype, F&& f) {
  if ((msg_dtype != 0 && msg_dtype != 1) || (w_dtype != 0 && w_dtype != 1)) return hipErrorInvalidValue;
  if (msg_dtype == 0) return w_dtype == 0 ? f(double{}, double{}) : f(double{}, float{});
  return w_dtype == 0 ? f(float{}, double{}) : f(float{}, float{});
}

template <class C>
hipError_t launch_blocked(const CombineArgs& args, int msg_dtype, int w_dtype, double* beta, double* u, double* hist,
                          void* beta_w, double* g_out, const C& bc, double theta, int rule, hipStream_t st,
                          long long* stamp) {
  if (bc.nblocks < 1 || bc.nblocks > kMaxBlocks || bc.block_ld < 1 || bc.d_x < 1 || bc.d_x > bc.block_ld)
    return hipErrorInvalidValue;
  return dispatch_msg_w(msg_dtype, w_dtype, [&](auto m, auto w) {
    using M = decltype(m);
    using W = decltype(w);
    hipLaunchKernelGGL((combine_update_blocked<M, W, C>), dim3(ceil_div(bc.nblocks * bc.block_ld, 256)), dim3(256), 0,
                       st, args, bc, beta, u, hist, static_cast<W*>(beta_w), g_out, theta, rule, stamp);
    return hipGetLastError();
  });
}

}  // namespace

// The launchers stand in this order (prox, blocks, combine_update) because the kernels are emitted in the order of
// their first use: combine_update's instantiations then close the object's text as they always did (placed
// elsewhere, the last of them gains a line of zero fill behind its s_endpgm, which tools/isa_diff.py counts).
hipError_t combine_update_prox_launch(const CombineArgs& args, int msg_dtype, int w_dtype, double* beta, double* u,
                                      double* hist, void* beta_w, double* g_out, const ProxCoefs& pc, double theta,
                                      int rule, hipStream_t st, long long* stamp) {
  for (int k = 0; k < pc.nblocks && k < kMaxBlocks; ++k)
    if (!(pc.thr[k] >= 0.0)) return hipErrorInvalidValue;  // negative or NaN
  return launch_blocked(args, msg_dtype, w_dtype, beta, u, hist, beta_w, g_out, pc, theta, rule, st, stamp);
}

hipError_t combine_update_blocks_launch(const CombineArgs& args, int msg_dtype, int w_dtype, double* beta, double* u,
                                        double* hist, void* beta_w, double* g_out, const BlockCoefs& bc, double theta,
                                        int rule, hipStream_t st, long long* stamp) {
  return launch_blocked(args, msg_dtype, w_dtype, beta, u, hist, beta_w, g_out, bc, theta, rule, st, stamp);
}

// msg dtype: 0 fp64, 1 fp32; worker beta dtype: 0 fp64, 1 fp32
hipError_t combine_update_launch(const CombineArgs& args, int msg_dtype, int w_dtype,
                                 double* beta, double* u, double* hist, void* beta_w,
                                 double* g_out, int d, int ld, double decay, double gm,
                                 double l2, double theta, int rule, hipStream_t st, long long* stamp) {
  return dispatch_msg_w(msg_dtype, w_dtype, [&](auto m, auto w) {
    using M = decltype(m);
    using W = decltype(w);
    hipLaunchKernelGGL((combine_update<M, W>), dim3(ceil_div(ld, 256)), dim3(256), 0, st, args, beta, u, hist,
                       static_cast<W*>(beta_w), g_out, d, ld, decay, gm, l2, theta, rule, stamp);
    return hipGetLastError();
  });
}

__global__ void stamp_kernel(long long* out) {
  if (threadIdx.x == 0) *out = wall_clock64();
}

hipError_t stamp_launch(long long* out, hipStream_t st) {
  hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(64), 0, st, out);
  return hipGetLastError();
}

}  // namespace eh
