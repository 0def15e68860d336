// Gradient and Hessian diagonal of one scalar-loss model in one pass over X: the worker kernel of a Jacobi-
// preconditioned (diagonal-Newton) run (--precondition diag).
//
// The objective is (1/n) sum_i l_i + alpha |beta|^2.  For a row x with label y, z = x . beta and t = y z:
//     loss            residual r (coefficient 1)              curvature w = l''(z)
//     logistic        -y s,  s = sigmoid(-t)                   s (1 - s)
//     least squares   -2 (y - z)                               2
//     squared hinge   -2 y max(0, 1 - t)                       2 where t < 1, else 0
// and partition p gives  g_p = sum r_i x_i  and  h_p = sum w_i x_i^2  (element-wise square).  Both are linear in the
// partitions, so a worker message is sum c_p [g_p ; h_p] with the gradient code's own coefficients: a blocked vector
// [2][ld] (grad_blocks.h), block 0 the gradient, block 1 the curvature diagonal.  The model on the wire has the same
// shape, block 0 beta and block 1 exact zeros; this kernel reads block 0 only.
//
// The master divides by the decoded diagonal (update.hip combine_update_precond):
//     P_j = gs max(h_j, 0) + 2 alpha + damping,   beta'_j = beta_j - eta (gs g_j + 2 alpha beta_j) / P_j.
//
// Transport: the blocked-model one as it stands -- a workgroup of kBlockSubs = 4 waves per task, the two-stage LDS
// ring fed by LDS-DMA (nt), blocks_stage_rows / blocks_ring_bytes, one barrier per stage, blocks_reduce behind it.
// The row loop is this kernel's own.  grad_models_kernel.h is built around two models per wave (two dot products, a
// two-value reduce-scatter, readlane of lanes 0 and 32); here there is ONE model and TWO accumulator sets:
//   * all four waves split a stage's rows, wave w takes rows w, w + 4, ...;
//   * a wave holds beta, g and h in registers: 3 CPL accumulator values per lane, plus the row;
//   * per row: the row from LDS once into registers (clamped read past the row end, beta is 0 there), one dot
//     product, one full-wave reduction, r and w together from the reduced z (logistic: from the one sigmoid, no
//     second exp), both broadcast with readlane, then g = fma(r, e, g) and h = fma(w e, e, h) from the same registers;
//   * no LDS besides the ring.
// Wave w stores g to slab row [task][w][0][.] and h to [task][w][1][.]; blocks_wpg(2) = 4 slab rows per task of
// D = 2 ld elements is what BlockGradPlan allocates, and blocks_reduce adds them in a fixed order (no atomics:
// bitwise reproducible) with exact zeros in the padding columns of both blocks.
#include "common.h"
#include "grad_blocks.h"
#include "grad_dense.h"
#include "launchers.h"
#include "lds_dma.h"

namespace eh {

namespace {

constexpr int kCurvBlocks = 2;  // [gradient ; curvature diagonal]

}  // namespace

template <typename T, typename A, int CPL, int LOSS>
__global__ void __launch_bounds__(256, 2)
grad_curv(const Segment* __restrict__ segs, const Task* __restrict__ tasks, const A* __restrict__ beta,
          A* __restrict__ slab, int blocks, int ld, int srows, const int* __restrict__ gate) {
  constexpr int VN = Vec16<T>::N;
  constexpr int NV = CPL / VN;
  using Rw = typename Vec16<T>::raw;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if (gate_closed(gate)) return;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lds_base = static_cast<unsigned>(
      reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char*)smem_raw));
  const int rowbytes = ld * static_cast<int>(sizeof(T));
  const int data_bytes = (srows * rowbytes + 1023) / 1024 * 1024;  // one stage: data, then 256 B of labels
  const int buf_bytes = data_bytes + 256;

  A b[NV][VN], g[NV][VN], h[NV][VN];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c0 = (j * kWave + lane) * VN;
#pragma unroll
    for (int v = 0; v < VN; ++v) {
      b[j][v] = c0 < ld ? beta[c0 + v] : A(0);  // block 0 of the model; block 1 is not read
      g[j][v] = h[j][v] = A(0);
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
      Rw xr[NV];  // the row, read once: the dot product and both accumulator sets use it
      A z = A(0);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        // clamped read past the row end: beta is 0 there, so the terms add exactly 0
        const int c0 = min((j * kWave + lane) * VN, ld - VN) * static_cast<int>(sizeof(T));
        xr[j] = *reinterpret_cast<const Rw*>(row + c0);
#pragma unroll
        for (int v = 0; v < VN; ++v) z = fma(Vec16<T>::template elem<A>(xr[j], v), b[j][v], z);
      }
      z = wave_allreduce_sum(z);  // the same bits on every lane
      A r, cw;
      residual_curvature<LOSS, A>(z, lab[i], r, cw);
      const A rs = readlane_a(r, 0), ws = readlane_a(cw, 0);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int v = 0; v < VN; ++v) {
          const A e = Vec16<T>::template elem<A>(xr[j], v);  // columns past the row end: never written
          g[j][v] = fma(rs, e, g[j][v]);
          h[j][v] = fma(ws * e, e, h[j][v]);
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
        out[ld + c0 + v] = h[j][v];
      }
    }
  }
}

hipError_t grad_curv_launch(int dtype, int loss, const void* segs, const void* tasks, int ntasks,
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
        // the weighted codes have no curvature instance: the range check above rejects them
        if constexpr (LOSS > kSquaredHinge) {
          return hipErrorInvalidValue;
        } else {
          const int rowbytes = ld_x * static_cast<int>(sizeof(T));
          const int srows = blocks_stage_rows(rowbytes);
          const size_t lds = blocks_ring_bytes(srows, rowbytes);
          auto launch = [&](auto kern) {
            return launch_blocks<A>(kern, lds, srows, kCurvBlocks, segs, tasks, ntasks, part_task_begin, nparts, beta,
                                    slab, Gb, d_x, ld_x, st, gate);
          };
          return ld_x <= 256   ? launch(grad_curv<T, A, 4, LOSS>)
                 : ld_x <= 512 ? launch(grad_curv<T, A, 8, LOSS>)
                               : launch(grad_curv<T, A, 16, LOSS>);
        }
      });
    }
  });
}

}  // namespace eh
