// Slab reduction of the dense worker gradient (host entry points: slab_reduce.h): the gradient kernels
// (grad_dense.hip, grad_mfma.hip) write one slab row per task; the kernels here sum the rows of every message in a
// fixed order, optionally with the worker's message put (put_protocol.h) or a local round's combine + update.
#include "common.h"
#include "integrity.h"
#include "launchers.h"
#include "put_protocol.h"
#include "slab_reduce.h"

namespace eh {

// Slab reduction, two fixed-order stages (bitwise reproducible, no atomics):
//   stage 1: block (64-column chunk, slot, split) — 4 waves stride over the split's tasks,
//            lane = column, then fold the waves in LDS -> part[slot][split][c]
//   stage 2: G[slot][c] = sum over splits of part[slot][split][c]
// 16 splits x 16 column chunks x slots gives thousands of workgroups for what used to be
// a 32-workgroup serial loop (70 us -> a few us at 2048 tasks x 1000 columns).
constexpr int kSplits = static_cast<int>(kSlabSplits);  // the int the kernels index with
// Slab reduction form of the non-update paths (set_slab_reduce_mode, for same-box A/B by bench.py
// --slab-mode and tools/bench_rank_shapes.py --slab-mode): 1 = one fused launch for plain reductions
// and puts (slab_reduce_fused[_put]); 2 = fused plain reductions, puts as stage 1 + the put kernel;
// 0 = the two stages everywhere.
static int g_slab_mode = 1;

template <typename A>
__global__ void __launch_bounds__(256)
slab_reduce_partial(const A* __restrict__ slab, const int* __restrict__ slot_task_begin,
                    A* __restrict__ part, int ld, const int* __restrict__ gate) {
  __shared__ A red[4][kWave];
  if (gate_closed(gate)) return;
  const int slot = blockIdx.y, split = blockIdx.z;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = blockIdx.x * kWave + lane;
  const int tb = slot_task_begin[slot], te = slot_task_begin[slot + 1];
  const int per = (te - tb + kSplits - 1) / kSplits;
  const int t0 = tb + split * per;
  const int t1 = min(te, t0 + per);
  A s = A(0);
  if (c < ld)
    for (int t = t0 + wid; t < t1; t += 4) s += slab[static_cast<long long>(t) * ld + c];
  red[wid][lane] = s;
  __syncthreads();
  if (wid == 0 && c < ld)
    part[(static_cast<long long>(slot) * kSplits + split) * ld + c] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

template <typename A>
__global__ void __launch_bounds__(256)
slab_reduce_final(const A* __restrict__ part, A* __restrict__ G, int ld, const int* __restrict__ gate) {
  const int slot = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ld || gate_closed(gate)) return;
  A s = A(0);
#pragma unroll
  for (int k = 0; k < kSplits; ++k) s += part[(static_cast<long long>(slot) * kSplits + k) * ld + c];
  G[static_cast<long long>(slot) * ld + c] = s;
}

// Both stages in ONE launch, bitwise the same sums: a 1024-thread block per (64-column chunk, slot),
// wave k = split k.  Lane c of wave k keeps the four interleaved sums stage 1's waves kept (rows
// t0 + w, t0 + w + 4, ... of its split, each in row order; eight rows loaded per step), folds them
// as (s0 + s1) + (s2 + s3), and wave 0 adds the 16 splits in order from A(0) like stage 2.  One launch
// and no partial buffer in HBM instead of two back-to-back launches (5.7 + 4.7 us at the 8-GPU rank
// shape, profiles/round4/prof_shape8).
template <typename A>
__device__ __forceinline__ A fused_split_sum(const A* __restrict__ slab, int t0, int t1, int ld, int c) {
  A acc[4] = {A(0), A(0), A(0), A(0)};
  int t = t0;
  for (; t + 8 <= t1; t += 8) {
    A v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = slab[static_cast<long long>(t + j) * ld + c];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j & 3] += v[j];  // accumulator (t - t0) % 4, rows in order
  }
  for (; t < t1; ++t) acc[(t - t0) & 3] += slab[static_cast<long long>(t) * ld + c];
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

template <typename A>
__device__ __forceinline__ A fused_slab_sum(const A* __restrict__ slab, const int* __restrict__ slot_task_begin,
                                            A (*red)[kWave], int slot, int ld, int c) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  const int tb = slot_task_begin[slot], te = slot_task_begin[slot + 1];
  const int per = (te - tb + kSplits - 1) / kSplits;
  const int t0 = tb + k * per;
  const int t1 = min(te, t0 + per);
  red[k][lane] = c < ld && t0 < t1 ? fused_split_sum(slab, t0, t1, ld, c) : A(0);
  __syncthreads();
  A s = A(0);
  if (k == 0)
#pragma unroll
    for (int q = 0; q < kSplits; ++q) s += red[q][lane];
  return s;  // meaningful in wave 0
}

template <typename A>
__global__ void __launch_bounds__(1024)
slab_reduce_fused(const A* __restrict__ slab, const int* __restrict__ slot_task_begin, A* __restrict__ G, int ld,
                  const int* __restrict__ gate) {
  __shared__ A red[kSplits][kWave];
  if (gate_closed(gate)) return;
  const int slot = blockIdx.y, c = blockIdx.x * kWave + (threadIdx.x & 63);
  const A s = fused_slab_sum(slab, slot_task_begin, red, slot, ld, c);
  if ((threadIdx.x >> 6) == 0 && c < ld) G[static_cast<long long>(slot) * ld + c] = s;
}

// The same with the worker's message put (put_protocol.h): every block also stores its sums straight
// into the receiver's mailbox rows (put.dst, the same [slot][ld] layout as G) and, for a tagged put,
// adds its columns' checksum terms of its slot's row into put.csum[slot].  Saves the separate
// put_signal launch on every worker round's critical path.  put.abort set: G is still written (the
// local copy) but nothing is put or announced.
template <typename A>
__global__ void __launch_bounds__(1024)
slab_reduce_fused_put(const A* __restrict__ slab, const int* __restrict__ slot_task_begin, A* __restrict__ G, int ld,
                      PutDesc put) {
  __shared__ A red[kSplits][kWave];
  __shared__ int s_last, s_live;
  const int slot = blockIdx.y, c = blockIdx.x * kWave + (threadIdx.x & 63);
  const bool w0 = (threadIdx.x >> 6) == 0;
  if (put_skipped(put, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)) return;
  if (threadIdx.x == 0) s_live = put_is_live(put);
  const A s = fused_slab_sum(slab, slot_task_begin, red, slot, ld, c);  // (its barrier publishes s_live)
  const bool live = s_live;
  if (w0 && c < ld) {
    const long long o = static_cast<long long>(slot) * ld + c;
    G[o] = s;
    if (live) static_cast<A*>(put.dst)[o] = s;
  }
  if (!live) return;  // block-uniform
  if (put.tag && w0) {
    const unsigned long long ws = wave_sum_u64(c < ld ? tag_term(elem_bits(s), c) : 0ull);
    if (threadIdx.x == 0 && ws) atomicAdd(put.csum + slot, ws);
  }
  if (!put_block_is_last(put, gridDim.x * gridDim.y, &s_last)) return;  // block-uniform
  put_tags_from_csum(put, static_cast<int>(gridDim.y));
  put_publish(put);
}

// Stage 2 with the worker's message put, as slab_reduce_fused_put.  No early return before the
// count: every thread reaches the barriers.
template <typename A>
__global__ void __launch_bounds__(256)
slab_reduce_final_put(const A* __restrict__ part, A* __restrict__ G, int ld, PutDesc put) {
  __shared__ unsigned long long scratch[4];
  __shared__ int s_last, s_live;
  const int slot = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (put_skipped(put, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)) return;
  if (threadIdx.x == 0) s_live = put_is_live(put);
  __syncthreads();
  const bool live = s_live;
  unsigned long long term = 0;
  if (c < ld) {
    A s = A(0);
#pragma unroll
    for (int k = 0; k < kSplits; ++k) s += part[(static_cast<long long>(slot) * kSplits + k) * ld + c];
    const long long o = static_cast<long long>(slot) * ld + c;
    G[o] = s;
    if (live) static_cast<A*>(put.dst)[o] = s;
    term = tag_term(elem_bits(s), c);
  }
  if (!live) return;  // block-uniform
  if (put.tag) {
    const unsigned long long bs = block_sum_u64(term, scratch);
    if (threadIdx.x == 0 && bs) atomicAdd(put.csum + slot, bs);
  }
  if (!put_block_is_last(put, gridDim.x * gridDim.y, &s_last)) return;  // block-uniform
  put_tags_from_csum(put, static_cast<int>(gridDim.y));
  put_publish(put);
}

// Stage 2 + put of a SMALL message set (nslots * ld <= kPutOneElems: the 8-GPU rank's 3 x 1000) in
// ONE 1024-thread block: no cross-block counter and no second release -- the block sums its
// elements two at a time (32 split loads in flight per thread), keeps the tag checksums in LDS
// (integer adds, order-free), writes the tags, releases once and stores the flag.  The multi-block
// form pays a device-scope atomic round trip and the last block's own release on top.
constexpr int kPutOneElems = 4096, kPutOneSlots = 16;

template <typename A>
__global__ void __launch_bounds__(1024)
slab_reduce_final_put1(const A* __restrict__ part, A* __restrict__ G, int ld, int nslots, PutDesc put) {
  __shared__ unsigned long long tsum[kPutOneSlots];
  __shared__ int s_live;
  const int tid = threadIdx.x;
  if (put_skipped(put, tid == 0)) return;
  if (tid < kPutOneSlots) tsum[tid] = 0;
  if (tid == 0) s_live = put_is_live(put);
  __syncthreads();
  const bool live = s_live;
  const int n = nslots * ld;
  for (int e0 = tid; e0 < n; e0 += 2 * static_cast<int>(blockDim.x)) {
    const int e1 = e0 + static_cast<int>(blockDim.x);
    const int q0 = e0 / ld, c0 = e0 - q0 * ld;
    const bool two = e1 < n;
    const int q1 = two ? e1 / ld : q0, c1 = two ? e1 - q1 * ld : c0;
    A v0[kSplits], v1[kSplits];
#pragma unroll
    for (int k = 0; k < kSplits; ++k) {
      v0[k] = part[(static_cast<long long>(q0) * kSplits + k) * ld + c0];
      v1[k] = part[(static_cast<long long>(q1) * kSplits + k) * ld + c1];
    }
    A s0 = A(0), s1 = A(0);
#pragma unroll
    for (int k = 0; k < kSplits; ++k) {  // slab_reduce_final's order
      s0 += v0[k];
      s1 += v1[k];
    }
    G[e0] = s0;
    if (live) static_cast<A*>(put.dst)[e0] = s0;
    if (put.tag) atomicAdd(&tsum[q0], tag_term(elem_bits(s0), c0));
    if (two) {
      G[e1] = s1;
      if (live) static_cast<A*>(put.dst)[e1] = s1;
      if (put.tag) atomicAdd(&tsum[q1], tag_term(elem_bits(s1), c1));
    }
  }
  if (!live) return;  // block-uniform
  if (put.tag) {
    __syncthreads();
    if (tid < nslots) put.tag[tid] = MsgTag{static_cast<unsigned int>(put.value), put.rank, tsum[tid]};
  }
  put_publish(put);  // the rows, tags (and the landing stamp) before the flag
}

// Stage 2 + the master's combine and update of a device-driven local round in one launch
// (MasterPump::run_local; update.hip combine_update's arithmetic).  One block per 64-column chunk:
// its waves sum the chunk's splits for every slot (slab_reduce_final's order; G rows written, sums
// kept in LDS), then wave 0 combines the decoded messages in message order and updates beta / u /
// history / the next worker beta for those columns.  Replaces slab_reduce_final + combine_update
// (one launch less per round), results bitwise unchanged.  (A variant that also folded stage 1 in,
// with the last block of each chunk finishing it, paid a device-scope release fence per block --
// an L2 writeback on every XCD -- and took 427 us: profiles/round3/fused_update.)
// 1024 threads: 16 waves share a chunk's slots (the headline's 22 slots took ~6 dependent rounds of
// split loads per wave at 4 waves, 10.2 us per call: profiles/round3/prof_nt).
template <typename A>
__global__ void __launch_bounds__(1024)
slab_final_update(const A* __restrict__ part, A* __restrict__ G, int ld, int nslots, const LocalUpdate up) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lu_raw[];
  A* gs = reinterpret_cast<A*>(lu_raw);  // [nslots][64] the chunk's message sums
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = blockIdx.x * kWave + lane;
  if (up.stamp && blockIdx.x == 0 && threadIdx.x == 0) *up.stamp = wall_clock64();
  for (int q = wid; q < nslots; q += static_cast<int>(blockDim.x >> 6)) {
    A v = A(0);
    if (c < ld) {
#pragma unroll
      for (int k = 0; k < kSplits; ++k) v += part[(static_cast<long long>(q) * kSplits + k) * ld + c];
      G[static_cast<long long>(q) * ld + c] = v;
    }
    gs[q * kWave + lane] = v;
  }
  __syncthreads();
  if (wid != 0 || c >= ld) return;
  A* bw = static_cast<A*>(up.beta_w);
  if (c >= up.d) {  // padded columns stay exactly zero
    if (bw) bw[c] = A(0);
    return;
  }
  double g = 0.0;  // combine_update: the fma chain in message order
  for (int m = 0; m < up.nmsg; ++m) g = fma(up.coef[m], static_cast<double>(gs[up.slot[m] * kWave + lane]), g);
  const double b = up.beta[c];
  double nb;
  if (up.rule == 0) {  // GD
    nb = up.decay * b - up.gm * g;
  } else {  // AGD
    const double yt = (1.0 - up.theta) * b + up.theta * up.u[c];
    nb = yt - up.gm * g - up.l2 * b;
    up.u[c] = b + (nb - b) * (1.0 / up.theta);
  }
  up.beta[c] = nb;
  if (up.hist) up.hist[c] = nb;
  if (bw) bw[c] = static_cast<A>(nb);
}

// ---------------------------------------------------------------------------------
// Host launchers.
void set_slab_reduce_mode(int mode) { g_slab_mode = mode; }
int slab_reduce_mode() { return g_slab_mode; }

// The accumulator type of a launch's storage code (launchers.h storage_acc_code), chosen here for every
// entry point: f(A{}).
template <typename F>
static hipError_t with_acc(int dtype, F&& f) {
  if (!storage_code_ok(dtype)) return hipErrorInvalidValue;
  return storage_acc_code(dtype) == 0 ? f(double{}) : f(float{});
}

hipError_t slab_reduce_launch(int dtype, const void* slab_, const int* stb, void* part_, void* G_, int nslots, int ld,
                              hipStream_t st, const PutDesc* put, const int* gate) {
  if (put && put->tag && (nslots > kMaxTagRows || !put->csum)) return hipErrorInvalidValue;
  if (put && put->gate != gate) return hipErrorInvalidValue;  // one round, one gate
  PutDesc pd{};
  if (put) {  // the process's release form (launchers.h strict_release)
    pd = *put;
    pd.strict = strict_release() ? 1 : 0;
    put = &pd;
  }
  return with_acc(dtype, [&](auto acc) {
    using A = decltype(acc);
    const A* slab = static_cast<const A*>(slab_);
    A *part = static_cast<A*>(part_), *G = static_cast<A*>(G_);
    const dim3 fgrid(ceil_div(ld, kWave), nslots);
    if (g_slab_mode != 0 && !put) {  // both stages in one launch (bitwise the same sums)
      hipLaunchKernelGGL(slab_reduce_fused<A>, fgrid, dim3(1024), 0, st, slab, stb, G, ld, gate);
      return hipGetLastError();
    }
    if (g_slab_mode == 1 && put) {
      hipLaunchKernelGGL(slab_reduce_fused_put<A>, fgrid, dim3(1024), 0, st, slab, stb, G, ld, *put);
      return hipGetLastError();
    }
    hipLaunchKernelGGL(slab_reduce_partial<A>, dim3(ceil_div(ld, kWave), nslots, kSplits), dim3(256), 0, st,
                       slab, stb, part, ld, gate);
    if (put && nslots <= kPutOneSlots && static_cast<long long>(nslots) * ld <= kPutOneElems)
      hipLaunchKernelGGL(slab_reduce_final_put1<A>, dim3(1), dim3(1024), 0, st, part, G, ld, nslots, *put);
    else if (put)
      hipLaunchKernelGGL(slab_reduce_final_put<A>, dim3(ceil_div(ld, 256), nslots), dim3(256), 0, st, part, G, ld, *put);
    else
      hipLaunchKernelGGL(slab_reduce_final<A>, dim3(ceil_div(ld, 256), nslots), dim3(256), 0, st, part, G, ld, gate);
    return hipGetLastError();
  });
}

hipError_t slab_reduce_update_launch(int dtype, const void* slab, const int* stb, void* part, void* G, int nslots,
                                     int ld, hipStream_t st, const LocalUpdate& up) {
  return with_acc(dtype, [&](auto acc) {
    using A = decltype(acc);
    const size_t lds = static_cast<size_t>(nslots) * kWave * sizeof(A);
    hipLaunchKernelGGL(slab_reduce_partial<A>, dim3(ceil_div(ld, kWave), nslots, kSplits), dim3(256), 0, st,
                       static_cast<const A*>(slab), stb, static_cast<A*>(part), ld, nullptr);
    if (const hipError_t e = allow_dynamic_lds(slab_final_update<A>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(slab_final_update<A>, dim3(ceil_div(ld, kWave)), dim3(1024), lds, st,
                       static_cast<const A*>(part), static_cast<A*>(G), ld, nslots, up);
    return hipGetLastError();
  });
}

}  // namespace eh
