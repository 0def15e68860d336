// The put + announce protocol of the IPC mailbox (device code only), one copy for every kernel that writes a
// message into a receiver's memory and then tells the receiver so: transport.hip put_signal and the slab
// reductions that carry the worker's put (slab_reduce.hip).  One PutDesc (launchers.h) per launch (put_signal:
// per blockIdx.y); strict = PutDesc::strict, the process's release form (common.h block_release_system).
// The steps, in the order every such kernel runs them:
//  1 put_skipped         The stale-round gate is closed (launch-uniform, common.h gate_closed): the grid returns,
//                        nothing is put or announced; one thread still decides the NEXT round's gate (step 6).
//  2 put_is_live         The abort word, read ONCE per block by one thread and shared through LDS (every wave takes
//                        the same branch).  Set: the pump gave up, nothing is put or announced (G is still written).
//  3 (the kernel)        Payload stores into dst; a tagged put adds the block's checksum terms into csum[row].
//  4 put_block_is_last   block_release_system: every wave waits for its stores, the block joins, one lane writes
//                        the L2 back at system scope -- the block's rows (and checksum adds) are out BEFORE it
//                        counts itself done.  The count is relaxed (acq_rel when strict): the release already
//                        ordered the block's stores, and the last block reads only the checksum sums, which are
//                        L2 atomics.  The last block resets the counter for the next launch; the others return
//                        (the one-block slab_reduce_final_put1 has no step 4).
//  5 put_tags_from_csum  The last block turns the sums into the receiver's MsgTags and leaves the scratch zero.
//  6 put_publish         The corrupt test hook (a torn put: one payload byte flipped AFTER its checksum) and the
//                        landing stamp, then a second release: tags and stamp (one-block put: the rows too) are
//                        out BEFORE the flag, which one thread stores (publish_u64: relaxed behind the release,
//                        release-ordered when strict): a receiver that observes flag >= value also observes rows,
//                        tags and stamp, without relying on kernel-boundary cache semantics across devices.
//                        Last, the same thread decides the next round's gate.
#pragma once

#include "common.h"
#include "launchers.h"

namespace eh {

// The landing stamp of a put (one thread of the last block, before the release that precedes the flag).
__device__ __forceinline__ void put_stamp(const PutDesc& p) {
  if (!p.stamp && !p.stamp_log) return;
  const long long t = static_cast<long long>(wall_clock64());
  if (p.stamp) {
    p.stamp[0] = static_cast<long long>(p.value);
    p.stamp[1] = t;
  }
  if (p.stamp_log) *p.stamp_log = t;
}
// The next round's gate word (one thread of the launch calls it).
__device__ __forceinline__ void put_decide_next_gate(const PutDesc& p) {
  if (!p.next_gate) return;
  const unsigned long long b =
      __hip_atomic_load(const_cast<unsigned long long*>(p.beta_flag), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(p.next_gate, b >= p.stale_next ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Step 1; first_thread: true in exactly one thread of the launch.
__device__ __forceinline__ bool put_skipped(const PutDesc& p, bool first_thread) {
  if (!gate_closed(p.gate)) return false;
  if (first_thread) put_decide_next_gate(p);
  return true;
}
// Step 2: one thread of the block calls it and shares the answer.
__device__ __forceinline__ bool put_is_live(const PutDesc& p) {
  return !(p.abort && __hip_atomic_load(p.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
// Step 4, by every thread of every live block (block-uniform); s_last: a __shared__ int of the block.
__device__ __forceinline__ bool put_block_is_last(const PutDesc& p, unsigned int total_blocks, int* s_last) {
  block_release_system(p.strict);
  if (threadIdx.x == 0) {
    const unsigned int prev = count_block_done(p.counter, p.strict);
    *s_last = prev == total_blocks - 1;
    if (*s_last) __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return *s_last;
}
// Step 5, by every thread of the last block (every block's adds are in: each counted behind its release).
__device__ __forceinline__ void put_tags_from_csum(const PutDesc& p, int rows) {
  if (!p.tag) return;
  for (int r = threadIdx.x; r < rows; r += blockDim.x) {
    const unsigned long long sum = atomicExch(p.csum + r, 0ull);
    p.tag[r] = MsgTag{static_cast<unsigned int>(p.value), p.rank, sum};
  }
}
// Step 6, by every thread of the last (or only) block, after its tag stores.
__device__ __forceinline__ void put_publish(const PutDesc& p) {
  if (p.tag && p.corrupt && threadIdx.x == 0) static_cast<unsigned char*>(p.dst)[1] ^= 0x10;  // test hook
  if (threadIdx.x == 0) put_stamp(p);
  block_release_system(p.strict);
  if (threadIdx.x == 0) {
    publish_u64(p.flag, p.value, p.strict);
    put_decide_next_gate(p);
  }
}

}  // namespace eh
