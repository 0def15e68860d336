// Multi-class softmax (multinomial logistic) gradient: one pass over X for all C classes.
//
// Model B [C][ld] class-major, labels = class indices (floats in the accumulator type).  For a row x:
//   z_c = x . B_c,  p = softmax(z) (max subtracted before exp),  r_c = p_c - [y == c],  G_c += r_c x.
// One-vs-rest on the scalar-residual kernels would stream X once per class; here a workgroup streams
// a row range of one partition through a two-stage LDS ring with LDS-DMA (grad_dense_staged's
// transport: every X element leaves HBM once per launch, nt policy) and all C dot products, the
// softmax and all C gradient rows are formed from the LDS copy.
//
// Workgroup = 4 waves.  Classes are split into groups of two: a wave holds B and the gradient
// accumulators of its two classes in registers.  With C <= 4 fewer than four groups exist and the
// spare waves split each stage's rows instead (wpg = 4 / groups waves per group: C = 2 -> 4,
// C = 3, 4 -> 2, C >= 5 -> 1; with 3 groups the fourth wave idles but joins every barrier).  Per stage:
//   1. every wave forms its two classes' logits of its rows (one two-value reduce-scatter per row)
//      and lane 0 / lane 32 write them to a small LDS array z[row][8];
//   2. one barrier;
//   3. every wave evaluates the softmax of its rows with one (row, class) pair per lane -- one exp per
//      lane for eight rows, max and denominator as 8-lane DPP all-reduces -- and leaves the residuals of
//      its two classes in a second small LDS array (the per-lane-row form, C exps per lane for every
//      stage, made exp the largest share of the VALU instructions: docs/PERF_NOTES.md);
//   4. the wave re-reads each of its rows from LDS and accumulates r_c * x, the residuals read back as
//      LDS broadcasts.
// Labels are only ever compared with the class numbers, never used as an index.
// Every wave writes its partial sums to its own slab row [task][sub][C][ld]; blocks_reduce (grad_blocks.h) adds a
// partition's slab rows in a fixed order (no atomics: bitwise reproducible) and writes exact zeros
// into the padding columns [d_x, ld) of every class block.
#include "common.h"
#include "grad_blocks.h"
#include "grad_dense.h"
#include "launchers.h"
#include "lds_dma.h"

namespace eh {

namespace {

constexpr int kSmWaves = kBlockSubs;
constexpr int kSmZStride = 8;  // logits per row in LDS (kMaxBlocks)

}  // namespace

template <typename T, typename A, int CPL>
__global__ void __launch_bounds__(256)
grad_softmax(const Segment* __restrict__ segs, const Task* __restrict__ tasks, const A* __restrict__ beta,
             A* __restrict__ slab, int C, int ld, int srows, const int* __restrict__ gate) {
  constexpr int VN = Vec16<T>::N;
  constexpr int NV = CPL / VN;
  using Rw = typename Vec16<T>::raw;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if (gate_closed(gate)) return;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ngrp = (C + 1) >> 1;
  const int wpg = kSmWaves / ngrp;
  const int grp = w / wpg, sub = w % wpg;
  const int cA = 2 * grp, cB = cA + 1;
  const bool actA = cA < C, actB = cB < C;  // wave-uniform; actB implies actA
  const unsigned lds_base = static_cast<unsigned>(
      reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char*)smem_raw));
  const int rowbytes = ld * static_cast<int>(sizeof(T));
  const int data_bytes = (srows * rowbytes + 1023) / 1024 * 1024;  // one stage: data, then 256 B of labels
  const int buf_bytes = data_bytes + 256;
  A* zb = reinterpret_cast<A*>(smem_raw + 2 * buf_bytes);  // logits [srows][kSmZStride]
  A* rbuf = zb + srows * kSmZStride;                        // residuals [srows][kSmZStride]

  A bA[NV][VN], bB[NV][VN];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c0 = (j * kWave + lane) * VN;
#pragma unroll
    for (int v = 0; v < VN; ++v) {
      bA[j][v] = actA && c0 < ld ? beta[cA * ld + c0 + v] : A(0);
      bB[j][v] = actB && c0 < ld ? beta[cB * ld + c0 + v] : A(0);
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
    for (int blk = w; blk * 1024 < bytes; blk += kSmWaves)
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
    __syncthreads();  // every wave's pieces of stage t; stage t-1 (ring buffer and logits) consumed by every wave
    if (t + 1 < nst) issue(t + 1);  // into the buffer stage t-1 used
    const unsigned char* buf = smem_raw + (t & 1) * buf_bytes;
    const A* lab = reinterpret_cast<const A*>(buf + data_bytes);
    const int ns = min(srows, nrows - t * srows);
    if (actA) {
      const bool hi = lane >= 32;
      for (int i = sub; i < ns; i += wpg) {
        const unsigned char* row = buf + i * rowbytes;
        A zA = A(0), zB = A(0);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          // clamped read past the row end: B is 0 there, so the terms add exactly 0 (grad_dense_staged)
          const int c0 = min((j * kWave + lane) * VN, ld - VN) * static_cast<int>(sizeof(T));
          const Rw xr = *reinterpret_cast<const Rw*>(row + c0);
#pragma unroll
          for (int v = 0; v < VN; ++v) {
            const A e = Vec16<T>::template elem<A>(xr, v);
            zA = fma(e, bA[j][v], zA);
            zB = fma(e, bB[j][v], zB);
          }
        }
        const A zs = wave_pair_reduce(zA, zB, hi);  // lanes 0-31: class cA, lanes 32-63: class cB
        if (lane == 0) zb[i * kSmZStride + cA] = zs;
        if (lane == 32) zb[i * kSmZStride + cB] = zs;  // cB <= 7: inside the row's 8 slots even when idle
      }
    }
    __syncthreads();  // all C logits of the stage's rows
    if (actA) {
      // Softmax of this wave's rows, one (row, class) pair per lane: lanes 8k..8k+7 hold the 8 logit slots
      // of the wave's k-th row of the pass, so a row costs one exp per lane instead of C per lane.  Max and
      // denominator are 8-lane all-reduces in DPP moves (quad_perm xor 1 / xor 2, row_half_mirror).  The
      // two residuals of the wave's classes go to rbuf[row][8] (read back by this wave only).
      const int nrw = (ns - sub + wpg - 1) / wpg;  // this wave's rows in the stage
      const int cl = lane & 7;
      for (int q = 0; q * 8 < nrw; ++q) {
        const int k = q * 8 + (lane >> 3);
        const int il = sub + wpg * k;
        const bool live = k < nrw && cl < C;
        const A z = live ? zb[il * kSmZStride + cl] : -INFINITY;
        A m = z;
        m = fmax(m, dpp_mov<0xB1>(m));
        m = fmax(m, dpp_mov<0x4E>(m));
        m = fmax(m, dpp_mov<0x141>(m));
        const A e = live ? exp(z - m) : A(0);  // arguments <= 0 and one of them 0: 1 <= den <= C
        A den = e;
        den += dpp_mov<0xB1>(den);
        den += dpp_mov<0x4E>(den);
        den += dpp_mov<0x141>(den);
        if (live && (cl == cA || cl == cB)) {
          const A y = lab[il];
          rbuf[il * kSmZStride + cl] = e / den - (y == static_cast<A>(cl) ? A(1) : A(0));
        }
      }
      for (int i = sub; i < ns; i += wpg) {
        const A ra = rbuf[i * kSmZStride + cA], rb = actB ? rbuf[i * kSmZStride + cB] : A(0);
        const unsigned char* row = buf + i * rowbytes;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int c0 = min((j * kWave + lane) * VN, ld - VN) * static_cast<int>(sizeof(T));
          const Rw xr = *reinterpret_cast<const Rw*>(row + c0);
#pragma unroll
          for (int v = 0; v < VN; ++v) {
            const A e = Vec16<T>::template elem<A>(xr, v);  // columns past the row end: never written
            gA[j][v] = fma(ra, e, gA[j][v]);
            gB[j][v] = fma(rb, e, gB[j][v]);
          }
        }
      }
    }
  }
  if (actA) {
    A* out = slab + (static_cast<long long>(task.slab) * wpg + sub) * (static_cast<long long>(C) * ld);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c0 = (j * kWave + lane) * VN;
#pragma unroll
      for (int v = 0; v < VN; ++v) {
        if (c0 + v < ld) {
          out[cA * ld + c0 + v] = gA[j][v];
          if (actB) out[cB * ld + c0 + v] = gB[j][v];
        }
      }
    }
  }
}

hipError_t grad_softmax_launch(int dtype, int classes, const void* segs, const void* tasks, int ntasks,
                               const int* part_task_begin, int nparts, const void* beta, void* slab, void* Gb,
                               int d_x, int ld_x, hipStream_t st, const int* gate) {
  if (classes < kMinBlocks || classes > kMaxBlocks || ld_x < 1 || ld_x > kBlockMaxLd || d_x < 1 || d_x > ld_x ||
      (dtype != 0 && dtype != 1) || ld_x % storage_vec(dtype) != 0)
    return hipErrorInvalidValue;
  if (nparts == 0) return hipSuccess;
  return dispatch_storage(dtype, [&](auto S) {
    using T = typename decltype(S)::T;
    using A = typename decltype(S)::A;
    if constexpr (!std::is_same_v<T, A>) {  // no bf16 or fp32x64 instance
      return hipErrorInvalidValue;
    } else {
      const int rowbytes = ld_x * static_cast<int>(sizeof(T));
      const int srows = blocks_stage_rows(rowbytes);
      // behind the ring: the logits and the residuals of a stage, [srows][kSmZStride] each
      const size_t lds = blocks_ring_bytes(srows, rowbytes, 2 * static_cast<size_t>(srows) * kSmZStride * sizeof(A));
      auto launch = [&](auto kern) {
        return launch_blocks<A>(kern, lds, srows, classes, segs, tasks, ntasks, part_task_begin, nparts, beta, slab, Gb,
                                d_x, ld_x, st, gate);
      };
      return ld_x <= 256   ? launch(grad_softmax<T, A, 4>)
             : ld_x <= 512 ? launch(grad_softmax<T, A, 8>)
                           : launch(grad_softmax<T, A, 16>);
    }
  });
}

void blocks_geometry(int rowbytes, int blocks, int* stage_rows, int* wpg) {
  *stage_rows = blocks_stage_rows(rowbytes);
  *wpg = blocks_wpg(blocks);
}

}  // namespace eh
