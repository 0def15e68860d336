// Master-side decode-combine + one round of truncated Newton (Newton-CG) in ONE launch of ONE workgroup
// (--newton-cg J).
//
// The method (all fp64, one model of a scalar loss).  The model on the wire is [2][ld_x]: block 0 beta, block 1 the
// conjugate-gradient direction; every message is [2][ld_x]: block 0 the coded gradient g, block 1 the coded
// Hessian-vector product u (grad_hvp.hip).  Both decode with the same coefficients, eight messages at a time in
// message order with the fma chain of combine_update_precond, and
//     G = gs g + l2c beta,     H v = gs u + l2c v.
// An outer iteration solves H x = -G by at most J steps of linear CG, one worker round per step:
//   gradient round (phase 0; block 1 of the wire is exact zeros)
//       x = 0, rres = -G, dir = rres, rs = rres . rres, g0norm2 = rs, G0 = G; beta stays, the next model is
//       [beta ; dir], phase 1.  If rs is 0 or not finite: the GD step beta' = beta - eta G, phase stays 0.
//   CG round (phase 1)
//       kappa = dir . H dir.  Not finite or <= 0 (an approximate or a table decode can give one): the inner loop ends
//       with the x held -- beta' = beta + tau x, or the GD step from G0 if no CG step was taken in this iteration.
//       Otherwise a = rs / kappa, x += a dir, rres -= a H dir, rs' = rres . rres.  When rs' <= xi^2 g0norm2 (or rs'
//       is NaN) or the inner count reaches J: beta' = beta + tau x, the next model is [beta' ; 0], phase 0.
//       Otherwise dir = rres + (rs' / rs) dir and the next model is [beta ; dir].
// So an outer iteration costs 1 + (CG steps used) rounds, and hist repeats beta during the CG rounds; block 1 of
// every hist row is exact zeros, so scoring sees a single model.
//
// One workgroup of 256 threads, any d: thread t owns columns t, t + 256, ... in every pass, so the passes need no
// barrier between them besides the reductions' own.  A CG round holds two DEPENDENT reductions (kappa, then rs'):
// pass 1 decodes, stores H dir in the state's scratch row and reduces kappa; pass 2 advances x and rres and reduces
// rs'; pass 3 writes dir, beta, the wire model and the history row.  Every reduction is a butterfly per wave, then
// the four wave sums added through LDS in wave order by every thread: no atomics, bitwise reproducible.
//
// The state lives on the device and the kernel itself advances it, so no host value but the round's coefficients
// enters the kernel and a captured graph of the round replays unchanged (as lbfgs.hip):
//   state [5][ld_x] fp64   x (the accumulated step), rres (the CG residual), dir, G0 (the gradient at the outer
//                          iterate), and a scratch row that holds H dir between the passes of a CG round
//   scal  [2] fp64         rs, g0norm2
//   phase [4] int32        phase (0 gradient round next, 1 CG round next), CG steps taken in this outer iteration,
//                          the last round's mode (kNewton* below), outer iterations finished
#include <cmath>

#include "common.h"
#include "launchers.h"

namespace eh {

namespace {

constexpr int kNewtonThreads = 256;
constexpr int kNewtonWaves = kNewtonThreads / 64;

// Sum over the workgroup, the same bits in every thread: a butterfly of commutative adds per wave, then the wave sums
// in wave order.  `red` is this reduction's own LDS row (no barrier is needed to reuse another's).
__device__ __forceinline__ double newton_block_sum(double v, double* red, int lane, int wave) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kNewtonWaves; ++w) s += red[w];
  return s;
}

}  // namespace

template <typename M, typename W>
__global__ void __launch_bounds__(kNewtonThreads)
newton_cg_update(const CombineArgs args, const NewtonCoefs nc, double* __restrict__ beta, double* __restrict__ hist,
                 W* __restrict__ beta_w, double* __restrict__ state, double* __restrict__ scal,
                 int* __restrict__ phase, long long* __restrict__ stamp, const int* __restrict__ gate) {
  __shared__ double red[2][kNewtonWaves];

  if (gate_closed(gate)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (stamp && tid == 0) *stamp = wall_clock64();
  const int d = nc.d_x, ld = nc.ld_x;
  double* xs = state;
  double* rres = state + ld;
  double* dir = state + 2LL * ld;
  double* G0 = state + 3LL * ld;
  double* hv = state + 4LL * ld;
  const int ph = phase[0] == 1 ? 1 : 0;  // (a state from elsewhere: a gradient round)
  const int inner = ph ? phase[1] : 0, outer = phase[3];
  const double rs = scal[0], g0n = scal[1];

  // ---- pass 1: decode both blocks; G and rs (gradient round) or H dir and kappa (CG round) ----------------------
  double acc = 0.0;
  for (int c = tid; c < d; c += kNewtonThreads) {
    double g = 0.0, u = 0.0;
    constexpr int kBatch = 8;  // independent loads eight at a time, accumulated in message order
    for (int m0 = 0; m0 < args.nmsg; m0 += kBatch) {
      double vg[kBatch], vu[kBatch];
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        const M* msg = m0 + k < args.nmsg ? static_cast<const M*>(args.msg[m0 + k]) : nullptr;
        vg[k] = msg ? static_cast<double>(msg[c]) : 0.0;
        vu[k] = msg ? static_cast<double>(msg[ld + c]) : 0.0;
      }
#pragma unroll
      for (int k = 0; k < kBatch; ++k)
        if (m0 + k < args.nmsg) {
          g = fma(args.coef[m0 + k], vg[k], g);
          u = fma(args.coef[m0 + k], vu[k], u);
        }
    }
    if (ph == 0) {
      const double G = fma(nc.gs, g, nc.l2c * beta[c]);
      G0[c] = G;
      acc = fma(G, G, acc);
    } else {
      const double v = dir[c];
      const double Hv = fma(nc.gs, u, nc.l2c * v);
      hv[c] = Hv;
      acc = fma(v, Hv, acc);
    }
  }
  const double s1 = newton_block_sum(acc, red[0], lane, wave);

  // what the round does: wave-uniform, from values every thread holds with the same bits
  int mode;
  bool stepped = false;  // this round took a CG step
  double rs_new = rs;
  if (ph == 0) {
    mode = (isfinite(s1) && s1 > 0.0) ? kNewtonStart : kNewtonGdGradient;
    rs_new = s1;
  } else if (!(isfinite(s1) && s1 > 0.0)) {
    mode = inner == 0 ? kNewtonGdCurvature : kNewtonStepCurvature;
  } else {
    // ---- pass 2: the CG step and the second, dependent reduction ------------------------------------------------
    stepped = true;
    const double a = rs / s1;
    double acc2 = 0.0;
    for (int c = tid; c < d; c += kNewtonThreads) {
      xs[c] = fma(a, dir[c], xs[c]);
      const double r = fma(-a, hv[c], rres[c]);
      rres[c] = r;
      acc2 = fma(r, r, acc2);
    }
    rs_new = newton_block_sum(acc2, red[1], lane, wave);
    if (!(rs_new > nc.xi * nc.xi * g0n))  // (a NaN rs' ends the inner loop too)
      mode = kNewtonStepTolerance;
    else if (inner + 1 >= nc.J)
      mode = kNewtonStepCap;
    else
      mode = kNewtonContinue;
  }
  const bool gd = mode == kNewtonGdGradient || mode == kNewtonGdCurvature;
  const bool cont = mode == kNewtonStart || mode == kNewtonContinue;  // the next round is a CG round
  const double bt = mode == kNewtonContinue ? rs_new / rs : 0.0;

  // ---- pass 3: the direction, beta, the wire model, the history row ----------------------------------------------
  for (int c = tid; c < ld; c += kNewtonThreads) {
    if (hist) hist[ld + c] = 0.0;  // block 1 of every stored iterate: exact zeros
    if (c >= d) {  // padded columns stay exactly zero
      if (beta_w) beta_w[c] = beta_w[ld + c] = W(0);
      continue;
    }
    const double b = beta[c];
    double nb = b, nd = 0.0;
    if (mode == kNewtonStart) {
      const double G = G0[c];
      xs[c] = 0.0;
      rres[c] = -G;
      dir[c] = nd = -G;
    } else if (mode == kNewtonContinue) {
      dir[c] = nd = fma(bt, dir[c], rres[c]);
    } else if (gd) {
      nb = fma(-nc.eta, G0[c], b);
    } else {
      nb = fma(nc.tau, xs[c], b);
    }
    if (!cont) beta[c] = nb;
    if (hist) hist[c] = nb;
    if (beta_w) {
      beta_w[c] = static_cast<W>(nb);
      beta_w[ld + c] = static_cast<W>(nd);
    }
  }
  if (tid == 0) {
    if (mode == kNewtonStart) scal[1] = rs_new;
    if (cont) scal[0] = rs_new;
    phase[0] = cont ? 1 : 0;
    phase[1] = mode == kNewtonStart ? 0 : (stepped ? inner + 1 : inner);
    phase[2] = mode;
    phase[3] = cont ? outer : outer + 1;
  }
}

hipError_t newton_cg_update_launch(const CombineArgs& args, int msg_dtype, int w_dtype, double* beta, double* hist,
                                   void* beta_w, double* state, double* scal, int* phase, const NewtonCoefs nc,
                                   hipStream_t st, long long* stamp, const int* gate) {
  if (nc.J < 1 || nc.J > kNewtonMaxInner || nc.ld_x < 1 || nc.d_x < 1 || nc.d_x > nc.ld_x || !(nc.xi > 0.0) ||
      !std::isfinite(nc.xi) || !(nc.tau > 0.0) || !std::isfinite(nc.tau) || args.nmsg < 0 || args.nmsg > kMaxMsgs ||
      !beta || !state || !scal || !phase)
    return hipErrorInvalidValue;  // (a NaN xi or tau fails the comparison)
  if ((msg_dtype != 0 && msg_dtype != 1) || (w_dtype != 0 && w_dtype != 1)) return hipErrorInvalidValue;
  auto go = [&](auto m, auto w) {
    using M = decltype(m);
    using W = decltype(w);
    hipLaunchKernelGGL((newton_cg_update<M, W>), dim3(1), dim3(kNewtonThreads), 0, st, args, nc, beta, hist,
                       static_cast<W*>(beta_w), state, scal, phase, stamp, gate);
    return hipGetLastError();
  };
  if (msg_dtype == 0) return w_dtype == 0 ? go(double{}, double{}) : go(double{}, float{});
  return w_dtype == 0 ? go(float{}, double{}) : go(float{}, float{});
}

}  // namespace eh
