// Several independent scalar-loss models over the same rows: one pass over X for all M models.
//
// An (alpha, lr) sweep trains M models that differ only in their update coefficients; their gradients
// at a round differ only through beta.  Model B [M][ld] model-major, labels as for the scalar losses.
// For a row x and model k:   z_k = x . B_k,  r_k = residual<LOSS>(z_k, y, 1),  G_k += r_k x.
// Running the one-model kernels M times would stream X once per model; here a workgroup streams a row
// range of one partition through grad_softmax.hip's transport (two-stage LDS ring with LDS-DMA, nt
// policy: every X element leaves HBM once per launch) and all M dot products, residuals and gradient
// rows are formed from the LDS copy.
//
// Workgroup = 4 waves, models in groups of two per wave as grad_softmax splits its classes (wpg = 4 /
// groups waves per group: M = 2 -> 4, M = 3, 4 -> 2, M >= 5 -> 1; with 3 groups the fourth wave idles but
// joins every barrier; spare waves split each stage's rows).  A wave holds B and the gradient
// accumulators of its two models in registers.  Unlike softmax a wave needs nothing from the other
// waves: for each of its rows it reads the row from LDS ONCE into registers, forms both dot products
// (one two-value reduce-scatter), evaluates the residual on the reduced value, broadcasts the two
// residuals with readlane and feeds the gradient FMAs from the same registers.  No logits / residual
// arrays in LDS and one barrier per stage.
// Every wave writes its partial sums to its own slab row [task][sub][M][ld]; blocks_reduce (grad_blocks.h) adds a
// partition's slab rows in a fixed order (no atomics: bitwise reproducible) and writes exact zeros into
// the padding columns [d_x, ld) of every model block.
#include "common.h"
#include "grad_blocks.h"
#include "grad_dense.h"
#include "launchers.h"
#include "lds_dma.h"

namespace eh {

namespace {

constexpr int kMmWaves = kBlockSubs;

}  // namespace

template <typename T, typename A, int CPL, int LOSS>
__global__ void __launch_bounds__(256, 2)
grad_models(const Segment* __restrict__ segs, const Task* __restrict__ tasks, const A* __restrict__ beta,
            A* __restrict__ slab, int M, int ld, int srows, const int* __restrict__ gate) {
  constexpr int VN = Vec16<T>::N;
  constexpr int NV = CPL / VN;
  using Rw = typename Vec16<T>::raw;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if (gate_closed(gate)) return;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ngrp = (M + 1) >> 1;
  const int wpg = kMmWaves / ngrp;
  const int grp = w / wpg, sub = w % wpg;
  const int mA = 2 * grp, mB = mA + 1;
  const bool actA = mA < M, actB = mB < M;  // wave-uniform; actB implies actA
  const unsigned lds_base = static_cast<unsigned>(
      reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char*)smem_raw));
  const int rowbytes = ld * static_cast<int>(sizeof(T));
  const int data_bytes = (srows * rowbytes + 1023) / 1024 * 1024;  // one stage: data, then 256 B of labels
  const int buf_bytes = data_bytes + 256;

  A bA[NV][VN], bB[NV][VN];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c0 = (j * kWave + lane) * VN;
#pragma unroll
    for (int v = 0; v < VN; ++v) {
      bA[j][v] = actA && c0 < ld ? beta[mA * ld + c0 + v] : A(0);
      bB[j][v] = actB && c0 < ld ? beta[mB * ld + c0 + v] : A(0);
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
    for (int blk = w; blk * 1024 < bytes; blk += kMmWaves)
      glds16(src + min(blk * 1024 + lane * 16, bytes - 16), dst + blk * 1024);
    if (w == 0) {
      const int lb = ns * static_cast<int>(sizeof(A));
      glds4(Y + r0 * sizeof(A) + min(lane * 4, lb - 4), dst + data_bytes);
    }
  };

  A gA[NV][VN], gB[NV][VN];
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int v = 0; v < VN; ++v) gA[j][v] = gB[j][v] = A(0);

  if (nst > 0) issue(0);
  for (int t = 0; t < nst; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of stage t landed
    __syncthreads();  // every wave's pieces of stage t; stage t-1's ring buffer consumed by every wave
    if (t + 1 < nst) issue(t + 1);  // into the buffer stage t-1 used
    if (!actA) continue;
    const unsigned char* buf = smem_raw + (t & 1) * buf_bytes;
    const A* lab = reinterpret_cast<const A*>(buf + data_bytes);
    const int ns = min(srows, nrows - t * srows);
    const bool hi = lane >= 32;
    for (int i = sub; i < ns; i += wpg) {
      const unsigned char* row = buf + i * rowbytes;
      Rw xr[NV];  // the row, read once: the dot products and the gradient FMAs both use it
      A zA = A(0), zB = A(0);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        // clamped read past the row end: B is 0 there, so the terms add exactly 0 (grad_softmax)
        const int c0 = min((j * kWave + lane) * VN, ld - VN) * static_cast<int>(sizeof(T));
        xr[j] = *reinterpret_cast<const Rw*>(row + c0);
#pragma unroll
        for (int v = 0; v < VN; ++v) {
          const A e = Vec16<T>::template elem<A>(xr[j], v);
          zA = fma(e, bA[j][v], zA);
          zB = fma(e, bB[j][v], zB);
        }
      }
      const A zs = wave_pair_reduce(zA, zB, hi);  // lanes 0-31: model mA, lanes 32-63: model mB (same bits per half)
      const A r = residual<LOSS, A>(zs, lab[i], A(1));
      const A ra = readlane_a(r, 0), rb = readlane_a(r, 32);  // an idle mB accumulates into gB, never written
#pragma unroll
      for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int v = 0; v < VN; ++v) {
          const A e = Vec16<T>::template elem<A>(xr[j], v);  // columns past the row end: never written
          gA[j][v] = fma(ra, e, gA[j][v]);
          gB[j][v] = fma(rb, e, gB[j][v]);
        }
      }
    }
  }
  if (actA) {
    A* out = slab + (static_cast<long long>(task.slab) * wpg + sub) * (static_cast<long long>(M) * ld);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c0 = (j * kWave + lane) * VN;
#pragma unroll
      for (int v = 0; v < VN; ++v) {
        if (c0 + v < ld) {
          out[mA * ld + c0 + v] = gA[j][v];
          if (actB) out[mB * ld + c0 + v] = gB[j][v];
        }
      }
    }
  }
}

hipError_t grad_models_launch(int dtype, int loss, int models, const void* segs, const void* tasks, int ntasks,
                              const int* part_task_begin, int nparts, const void* beta, void* slab, void* Gb, int d_x,
                              int ld_x, hipStream_t st, const int* gate) {
  if (models < kMinBlocks || models > kMaxBlocks || ld_x < 1 || ld_x > kBlockMaxLd || d_x < 1 || d_x > ld_x ||
      (dtype != 0 && dtype != 1 && dtype != 3) || ld_x % storage_vec(dtype) != 0 || loss < 0 || loss > kSquaredHinge)
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
        // the weighted codes (kLogisticW, kSquaredHingeW) have no multi-model instance: the range check above
        // rejects them, and nothing is instantiated for them here
        if constexpr (LOSS > kSquaredHinge) {
          return hipErrorInvalidValue;
        } else {
          const int rowbytes = ld_x * static_cast<int>(sizeof(T));
          const int srows = blocks_stage_rows(rowbytes);
          const size_t lds = blocks_ring_bytes(srows, rowbytes);
          auto launch = [&](auto kern) {
            return launch_blocks<A>(kern, lds, srows, models, segs, tasks, ntasks, part_task_begin, nparts, beta,
                                    slab, Gb, d_x, ld_x, st, gate);
          };
          return ld_x <= 256   ? launch(grad_models<T, A, 4, LOSS>)
                 : ld_x <= 512 ? launch(grad_models<T, A, 8, LOSS>)
                               : launch(grad_models<T, A, 16, LOSS>);
        }
      });
    }
  });
}

}  // namespace eh
