// What the blocked-model gradient kernels share (grad_softmax.hip: blocks = classes, grad_multimodel.hip: blocks =
// models): the geometry of their LDS ring, the fixed-order slab reduction and the launch of the two.
//
// The model and every Gb row are [blocks][ld] flattened to D = blocks * ld.  A workgroup of kBlockSubs waves streams
// a row range of one partition through a two-stage ring; blocks are held two per wave, and with fewer than four
// pairs the spare waves split each stage's rows, so a task leaves blocks_wpg(blocks) slab rows [task][sub][D].
#pragma once

#include <algorithm>

#include "common.h"
#include "grad_dense.h"
#include "launchers.h"

namespace eh {

// rows per LDS stage: about 32 KiB, at least one row per wave, at most 32 (the labels of a stage are one
// 256-byte LDS-DMA piece)
inline int blocks_stage_rows(int rowbytes) { return std::min(32, std::max(4, 32768 / rowbytes)); }
// the ring: data (whole KiB), then 256 B of labels, twice; extra: what a kernel keeps in LDS besides
inline size_t blocks_ring_bytes(int srows, int rowbytes, size_t extra = 0) {
  const size_t data = (static_cast<size_t>(srows) * rowbytes + 1023) / 1024 * 1024;
  return 2 * (data + 256) + extra;
}
// waves that share one pair of blocks: 2 blocks -> 4, 3 or 4 -> 2, 5..8 -> 1
constexpr int blocks_wpg(int blocks) { return kBlockSubs / ((blocks + 1) / 2); }

// Gb[p][e] = sum of partition p's slab rows (tasks in table order, waves in order) for element e of the
// [blocks][ld] vector; padding columns are exact zeros.  No atomics: bitwise reproducible.
template <typename A>
__global__ void __launch_bounds__(256)
blocks_reduce(const A* __restrict__ slab, const int* __restrict__ part_task_begin, A* __restrict__ Gb, int D,
              int d_x, int ld, int wpg, const int* __restrict__ gate) {
  const int p = blockIdx.y;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= D || gate_closed(gate)) return;
  A s = A(0);
  if (e % ld < d_x) {
    const long long r0 = static_cast<long long>(part_task_begin[p]) * wpg;
    const long long r1 = static_cast<long long>(part_task_begin[p + 1]) * wpg;
    const A* __restrict__ col = slab + e;
    for (long long r = r0; r < r1; ++r) s += col[r * D];
  }
  Gb[static_cast<long long>(p) * D + e] = s;
}

// kern (grad_softmax / grad_models: one workgroup per task, `lds` bytes of dynamic LDS, stages of srows rows), then
// the reduction of its slab rows into Gb [nparts][blocks * ld].
template <typename A, class K>
hipError_t launch_blocks(K kern, size_t lds, int srows, int blocks, const void* segs, const void* tasks, int ntasks,
                         const int* ptb, int nparts, const void* beta, void* slab, void* Gb, int d_x, int ld,
                         hipStream_t st, const int* gate) {
  if (const hipError_t e = allow_dynamic_lds(kern, lds); e != hipSuccess) return e;
  if (ntasks > 0)
    hipLaunchKernelGGL(kern, dim3(ntasks), dim3(64 * kBlockSubs), lds, st, static_cast<const Segment*>(segs),
                       static_cast<const Task*>(tasks), static_cast<const A*>(beta), static_cast<A*>(slab), blocks, ld,
                       srows, gate);
  const int D = blocks * ld;
  hipLaunchKernelGGL(blocks_reduce<A>, dim3(ceil_div(D, 256), nparts), dim3(256), 0, st, static_cast<const A*>(slab),
                     ptb, static_cast<A*>(Gb), D, d_x, ld, blocks_wpg(blocks), gate);
  return hipGetLastError();
}

}  // namespace eh
