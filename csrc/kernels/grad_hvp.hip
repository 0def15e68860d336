// Gradient and Hessian-vector product of one scalar-loss model in one pass over X: the worker kernel of a truncated
// Newton (Newton-CG) run (--newton-cg J).
//
// The model on the wire is [2][ld]: block 0 beta, block 1 the conjugate-gradient direction v (exact zeros in a
// gradient round).  For a row x with label y, z = x . beta, q = x . v and (r, w) = residual_curvature<LOSS>(z, y)
// (common.h: residual and l''(z) from one sigmoid).  Partition p gives
//     g_p = sum r_i x_i          (the gradient)
//     u_p = sum (w_i q_i) x_i    (the loss Hessian applied to v:  H v = sum w_i (x_i . v) x_i)
// Both are linear in the partitions, so a worker message is sum c_p [g_p ; u_p] with the gradient code's own
// coefficients: a blocked vector [2][ld] (grad_blocks.h), block 0 the gradient and block 1 the product.  The master
// (newton_cg.hip) adds the L2 term: G = gs g + l2c beta, H v = gs u + l2c v.
//
// Transport: the blocked-model one as it stands -- a workgroup of kBlockSubs = 4 waves per task, the two-stage LDS
// ring fed by LDS-DMA (nt), blocks_stage_rows / blocks_ring_bytes, one barrier per stage, blocks_reduce behind it.
// The row loop is this kernel's own:
//   * all four waves split a stage's rows, wave w takes rows w, w + 4, ...;
//   * a wave holds beta, v, g and u in registers: 4 CPL accumulator values per lane, plus the row;
//   * per row: the row from LDS once into registers (clamped read past the row end: beta AND v are loaded as 0 there,
//     so the terms of both dot products add exactly 0), both dot products from those registers, ONE two-value
//     reduce-scatter (wave_pair_reduce: lanes 0-31 end with z, lanes 32-63 with q), z and q read back with readlane,
//     r and w from the one sigmoid, r and w q broadcast with readlane, then g = fma(r, e, g) and u = fma(wq, e, u)
//     from the same registers;
//   * v = 0 gives q = +-0 and w q = +-0 exactly (w is finite), so block 1 is exact zeros in a gradient round;
//   * no LDS besides the ring.
// Wave w stores g to slab row [task][w][0][.] and u to [task][w][1][.]; blocks_wpg(2) = 4 slab rows per task of
// D = 2 ld elements is what BlockGradPlan allocates, and blocks_reduce adds them in a fixed order (no atomics:
// bitwise reproducible) with exact zeros in the padding columns of both blocks.
//
// Register budget.  __launch_bounds__(256, 2) is two workgroups per CU, two waves per SIMD: 256 registers per lane
// (VGPR + AGPR).  fp64 at CPL = 16 holds 4 x 16 doubles = 128 registers of beta, v, g, u and 32 of the row, 160 of
// the 256 before temporaries, so all four sets stay in one wave and no split of g and u over waves is needed.  What
// the compiler reports for gfx950 (hipcc -Rpass-analysis=kernel-resource-usage), VGPRs for logistic / least squares /
// squared hinge; every instance has 0 AGPRs and 0 bytes of scratch:
//     storage, accumulator    CPL 16           CPL 8           CPL 4
//     fp64, fp64           220 / 194 / 200  124 / 98 / 104  78 / 52 / 58
//     fp32, fp64 (x64)     208 / 180 / 188  118 / 90 /  94  78 / 50 / 58
//     fp32, fp32            99 /  93 /  95   53 / 47 /  49  33 / 27 / 29
// The largest, fp64 / CPL 16 / logistic, takes 220 of the 256.
#include "common.h"
#include "grad_blocks.h"
#include "grad_dense.h"
#include "launchers.h"
#include "lds_dma.h"

namespace eh {

namespace {

constexpr int kHvpBlocks = 2;  // [gradient ; Hessian-vector product], and the model's [beta ; v]

}  // namespace

template <typename T, typename A, int CPL, int LOSS>
__global__ void __launch_bounds__(256, 2)
grad_hvp(const Segment* __restrict__ segs, const Task* __restrict__ tasks, const A* __restrict__ beta,
         A* __restrict__ slab, int blocks, int ld, int srows, const int* __restrict__ gate) {
  constexpr int VN = Vec16<T>::N;
  constexpr int NV = CPL / VN;
  using Rw = typename Vec16<T>::raw;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if (gate_closed(gate)) return;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool hi = lane >= 32;
  const unsigned lds_base = static_cast<unsigned>(
      reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char*)smem_raw));
  const int rowbytes = ld * static_cast<int>(sizeof(T));
  const int data_bytes = (srows * rowbytes + 1023) / 1024 * 1024;  // one stage: data, then 256 B of labels
  const int buf_bytes = data_bytes + 256;

  A b[NV][VN], dv[NV][VN], g[NV][VN], u[NV][VN];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c0 = (j * kWave + lane) * VN;
#pragma unroll
    for (int v = 0; v < VN; ++v) {
      b[j][v] = c0 < ld ? beta[c0 + v] : A(0);        // block 0 of the model: beta
      dv[j][v] = c0 < ld ? beta[ld + c0 + v] : A(0);  // block 1: the direction; both 0 past the row end
      g[j][v] = u[j][v] = A(0);
    }
  }
  const Task task = tasks[blockIdx.x];
  const Segment sg = segs[task.seg];
  const unsigned char* __restrict__ X = static_cast<const unsigned char*>(sg.X);
  const unsigned char* __restrict__ Y = static_cast<const unsigned char*>(sg.y);
  const int nrows = task.row_end - task.row_begin;
  const int nst = (nrows + srows - 1) / srows;

  auto issue = [&](int t) {
    const unsigned dst = lds_base + (t & 1) * buf_bytes;
    const long long r0 = task.row_begin + static_cast<long long>(t) * srows;
    const int ns = min(srows, static_cast<int>(task.row_end - r0));
    const int bytes = ns * rowbytes;
    const unsigned char* src = X + r0 * rowbytes;
    for (int blk = w; blk * 1024 < bytes; blk += kBlockSubs)
      glds16(src + min(blk * 1024 + lane * 16, bytes - 16), dst + blk * 1024);
    if (w == 0) {
      const int lb = ns * static_cast<int>(sizeof(A));
      glds4(Y + r0 * sizeof(A) + min(lane * 4, lb - 4), dst + data_bytes);
    }
  };

  if (nst > 0) issue(0);
  for (int t = 0; t < nst; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of stage t landed
    __syncthreads();  // every wave's pieces of stage t; stage t-1's ring buffer consumed by every wave
    if (t + 1 < nst) issue(t + 1);  // into the buffer stage t-1 used
    const unsigned char* buf = smem_raw + (t & 1) * buf_bytes;
    const A* lab = reinterpret_cast<const A*>(buf + data_bytes);
    const int ns = min(srows, nrows - t * srows);
    for (int i = w; i < ns; i += kBlockSubs) {
      const unsigned char* row = buf + i * rowbytes;
      Rw xr[NV];  // the row, read once: both dot products and both accumulator sets use it
      A z = A(0), q = A(0);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        // clamped read past the row end: beta and v are 0 there, so the terms add exactly 0
        const int c0 = min((j * kWave + lane) * VN, ld - VN) * static_cast<int>(sizeof(T));
        xr[j] = *reinterpret_cast<const Rw*>(row + c0);
#pragma unroll
        for (int v = 0; v < VN; ++v) {
          const A e = Vec16<T>::template elem<A>(xr[j], v);
          z = fma(e, b[j][v], z);
          q = fma(e, dv[j][v], q);
        }
      }
      const A zq = wave_pair_reduce(z, q, hi);  // lanes 0-31: x . beta, lanes 32-63: x . v (same bits per half)
      const A zs = readlane_a(zq, 0), qs = readlane_a(zq, 32);
      A r, cw;
      residual_curvature<LOSS, A>(zs, lab[i], r, cw);
      const A rs = readlane_a(r, 0), wq = readlane_a(cw * qs, 0);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int v = 0; v < VN; ++v) {
          const A e = Vec16<T>::template elem<A>(xr[j], v);  // columns past the row end: never written
          g[j][v] = fma(rs, e, g[j][v]);
          u[j][v] = fma(wq, e, u[j][v]);
        }
      }
    }
  }
  // every wave writes its slab row, a wave without rows its zeros: blocks_reduce adds all four
  A* out = slab + (static_cast<long long>(task.slab) * kBlockSubs + w) * (static_cast<long long>(blocks) * ld);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c0 = (j * kWave + lane) * VN;
#pragma unroll
    for (int v = 0; v < VN; ++v) {
      if (c0 + v < ld) {
        out[c0 + v] = g[j][v];
        out[ld + c0 + v] = u[j][v];
      }
    }
  }
}

hipError_t grad_hvp_launch(int dtype, int loss, const void* segs, const void* tasks, int ntasks,
                           const int* part_task_begin, int nparts, const void* beta, void* slab, void* Gb, int d_x,
                           int ld_x, hipStream_t st, const int* gate) {
  if (ld_x < 1 || ld_x > kBlockMaxLd || d_x < 1 || d_x > ld_x || (dtype != 0 && dtype != 1 && dtype != 3) ||
      ld_x % storage_vec(dtype) != 0 || loss < 0 || loss > kSquaredHinge)
    return hipErrorInvalidValue;
  if (nparts == 0) return hipSuccess;
  return dispatch_storage(dtype, [&](auto S) {
    using T = typename decltype(S)::T;
    using A = typename decltype(S)::A;
    if constexpr (std::is_same_v<T, bf16_t>) {
      return hipErrorInvalidValue;
    } else {
      return dispatch_loss(loss, [&](auto L) -> hipError_t {
        constexpr int LOSS = decltype(L)::value;
        // the weighted codes have no curvature: the range check above rejects them
        if constexpr (LOSS > kSquaredHinge) {
          return hipErrorInvalidValue;
        } else {
          const int rowbytes = ld_x * static_cast<int>(sizeof(T));
          const int srows = blocks_stage_rows(rowbytes);
          const size_t lds = blocks_ring_bytes(srows, rowbytes);
          auto launch = [&](auto kern) {
            return launch_blocks<A>(kern, lds, srows, kHvpBlocks, segs, tasks, ntasks, part_task_begin, nparts, beta,
                                    slab, Gb, d_x, ld_x, st, gate);
          };
          return ld_x <= 256   ? launch(grad_hvp<T, A, 4, LOSS>)
                 : ld_x <= 512 ? launch(grad_hvp<T, A, 8, LOSS>)
                               : launch(grad_hvp<T, A, 16, LOSS>);
        }
      });
    }
  });
}

}  // namespace eh
