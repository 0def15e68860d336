// The one text of the several-scalar-loss-models gradient kernel, compiled once per translation unit that includes
// it, under the name and with the label rule that unit sets before the #include:
//
//   EH_MODELS_KERNEL   the kernel's name (grad_multimodel.hip: grad_models, grad_ovr.hip: grad_ovr,
//                      grad_folds.hip: grad_folds)
//   EH_MODELS_OVR      false: every model sees the rows' own labels (an (alpha, lr) sweep);
//                      true:  one-vs-rest, labels are class indices and model k sees +1 where the index is k, else -1
//   EH_MODELS_FOLDS    (optional, default false) true: K-fold cross-validation with K = M, row i of a partition
//                      belongs to fold i mod M and model k does not see the rows of fold k (their residual is 0)
//
// One copy of the row loop; EH_MODELS_OVR changes the one line that picks the label, EH_MODELS_FOLDS adds the one
// line that drops a held-out row's residual (and the scalar fold counter that line reads).  The text is included, not
// called: moved into a __device__ __forceinline__ template, the same statements compile to the same opcodes in another
// operand order and register assignment in every grad_models instance (tools/isa_diff.py, docs/PERF_NOTES.md), and
// the existing kernels' instruction streams are not to move.  No include guard: one kernel per inclusion.
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
#if !defined(EH_MODELS_KERNEL) || !defined(EH_MODELS_OVR)
#error "define EH_MODELS_KERNEL (the kernel's name) and EH_MODELS_OVR (true / false) before including grad_models_kernel.h"
#endif
#ifndef EH_MODELS_FOLDS
#define EH_MODELS_FOLDS false
#endif

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
EH_MODELS_KERNEL(const Segment* __restrict__ segs, const Task* __restrict__ tasks, const A* __restrict__ beta,
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

  // cross-validation: the fold of a row is its index in the PARTITION (the segment) mod M, whatever task and stage it
  // falls into.  Wave-uniform and division-free in the loops: fs = fold of the stage's first row, advanced by
  // srows mod M per stage; a wave's rows start at fs + sub and step by wpg (all reduced mod M once, up here).
  [[maybe_unused]] int fs = 0, fstage = 0, fsub = 0, fstep = 0;
  if constexpr (EH_MODELS_FOLDS) {
    fs = task.row_begin % M;
    fstage = srows % M;
    fsub = sub % M;
    fstep = wpg % M;
  }

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
    [[maybe_unused]] int f = 0;  // the fold of row i of this stage
    if constexpr (EH_MODELS_FOLDS) {
      f = fs + fsub;
      f -= f >= M ? M : 0;
      fs += fstage;
      fs -= fs >= M ? M : 0;
    }
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
      A yk = lab[i];
      // one-vs-rest: the label model mA / mB sees is +1 for the rows of its own class and -1 for the others
      if constexpr (EH_MODELS_OVR) yk = yk == static_cast<A>(hi ? mB : mA) ? A(1) : A(-1);
      A r = residual<LOSS, A>(zs, yk, A(1));
      // cross-validation: model mA / mB does not train on the rows of its own fold (the row still feeds the FMAs, with 0)
      if constexpr (EH_MODELS_FOLDS) {
        r = f == (hi ? mB : mA) ? A(0) : r;
        f += fstep;
        f -= f >= M ? M : 0;
      }
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

}  // namespace eh
